/*
 * fold.c — collision exclusions from plain C (include/phyx_amd.h COLLISION EXCLUSIONS): chain.c's chain, longer, folded like an
 * accordion and dropped on its lower end, so that it piles up on itself.  Run twice:
 *   - with chain.c's shared negative group: no link collides with any other link, and the chain falls through itself;
 *   - with the neighbours excluded (phx_world_get_pins, then one pair per pin that joins two bodies): link i passes through links
 *     i - 1 and i + 1, which it overlaps at the hinge, and lands on every other link.
 * Per run it prints the number of link-link manifolds between neighbours and between non-neighbours at the end.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/fold.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o fold
 *   ./fold [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a neighbour manifold in either run, a link-link
 * manifold under the shared group, none between non-neighbours under the exclusions).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phyx_amd.h"

#define TRY(call)                                                                      \
    do {                                                                               \
        int st_ = (call);                                                              \
        if (st_ != PHX_OK) {                                                           \
            fprintf(stderr, "%s -> %d: %s\n", #call, st_, phx_last_error());           \
            return st_ == PHX_ERR_NO_DEVICE ? 3 : 1;                                   \
        }                                                                              \
    } while (0)

#define LINKS 24
#define SPACING 10.0f      /* hinge to hinge */
#define RISE 5.0f          /* a link's rise in the folded chain: it leans 30 degrees */

/* one run: `exclude` = 0 the shared group, 1 the neighbour exclusions; the two counts of link-link manifolds at the end */
static int run(int exclude, int steps, int* neighbours, int* others)
{
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 1000.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    /* links of 8 x 2 between hinges that alternate left and right of the axis x = 0, the lowest hinge 20 above the ground */
    const float run_x = sqrtf(SPACING * SPACING - RISE * RISE), lean = atan2f(RISE, run_x), pi = 3.14159265f;
    int32_t link[LINKS];
    for (int k = 0; k < LINKS; ++k) {
        link[k] = phx_world_add_body(world, 0.0f, 30.0f + RISE * ((float)k + 0.5f), k % 2 ? pi - lean : lean, 4.0f, 1.0f);
        if (link[k] < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    }
    phx_pin pins[LINKS - 1];
    const phx_vec2 near_end = { -SPACING / 2.0f, 0.0f }, far_end = { SPACING / 2.0f, 0.0f }, zero = { 0.0f, 0.0f };
    for (int k = 1; k < LINKS; ++k) {
        pins[k - 1].body1 = link[k]; pins[k - 1].anchor1 = near_end; pins[k - 1].impulse = zero;
        pins[k - 1].body2 = link[k - 1]; pins[k - 1].anchor2 = far_end;
    }
    TRY(phx_world_add_pins(world, pins, LINKS - 1, NULL));
    TRY(phx_world_set_pin_iterations(world, 32));

    if (!exclude) {
        phx_collision_filter no_self[LINKS];
        for (int k = 0; k < LINKS; ++k) { no_self[k].category = 1u; no_self[k].mask = 0xFFFFFFFFu; no_self[k].group = -1; }
        TRY(phx_world_set_collision_filters(world, link, no_self, LINKS, NULL));
    } else {
        /* collideConnected = false: the body pair of every pin that joins two bodies */
        int32_t np = 0;
        TRY(phx_world_pin_count(world, &np));
        phx_pin* got = (phx_pin*)malloc((size_t)np * sizeof *got);
        int32_t* pairs = (int32_t*)malloc(2 * (size_t)np * sizeof *pairs);
        if (!got || !pairs) return 1;
        TRY(phx_world_get_pins(world, got, np));
        int32_t count = 0;
        for (int k = 0; k < np; ++k)
            if (got[k].body2 >= 0) { pairs[2 * count] = got[k].body1; pairs[2 * count + 1] = got[k].body2; ++count; }
        TRY(phx_world_add_collision_exclusions(world, pairs, count, NULL));
        free(got); free(pairs);
    }

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    for (int s = 0; s < steps; ++s) TRY(phx_world_update(world, dt, &cfg));

    int32_t nm = 0;
    TRY(phx_world_counts(world, NULL, &nm, NULL, NULL));
    phx_manifold* m = (phx_manifold*)malloc((size_t)(nm > 0 ? nm : 1) * sizeof *m);
    if (!m) return 1;
    TRY(phx_world_get_manifolds(world, m, nm));
    *neighbours = 0; *others = 0;
    for (int i = 0; i < nm; ++i) {
        const int a = m[i].body1 - link[0], b = m[i].body2 - link[0];      /* (the links are numbered in a row) */
        if (a < 0 || a >= LINKS || b < 0 || b >= LINKS) continue;
        if (abs(a - b) == 1) ++*neighbours; else ++*others;
    }
    free(m);
    phx_world_destroy(world);
    return 0;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 300;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    int near_group = 0, far_group = 0, near_set = 0, far_set = 0;
    int st = run(0, steps, &near_group, &far_group);
    if (st) return st;
    st = run(1, steps, &near_set, &far_set);
    if (st) return st;
    printf("fold: shared group -1: %d neighbour manifolds, %d other link-link manifolds after %d steps\n", near_group, far_group, steps);
    printf("fold: neighbours excluded: %d neighbour manifolds, %d other link-link manifolds after %d steps\n", near_set, far_set, steps);
    if (near_group || far_group) { fprintf(stderr, "links of one negative group collided\n"); return 1; }
    if (near_set) { fprintf(stderr, "an excluded pair got a manifold\n"); return 1; }
    if (!far_set) { fprintf(stderr, "the chain fell through itself although only its neighbours are excluded\n"); return 1; }
    return 0;
}
