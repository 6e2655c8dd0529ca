/*
 * place.c — the emitter that looks first, through the C ABI: every frame it asks phx_world_query_boxes whether the spawn slot is free
 * for the next box and spawns (phx_world_add_bodies) only then, so nothing is ever created inside another body.  The boxes pile up
 * under the slot until the pile reaches it; from then on every request is refused.  At the end one box is dropped straight down onto
 * the pile with phx_world_cast_boxes, which says how far it can fall before it touches something.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/place.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o place
 *   ./place [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or a spawn into an occupied slot).
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

/* the query box {pos, xv, yv, h} of a box at `angle` */
static void box_at(float x, float y, float angle, float hx, float hy, float* q)
{
    q[0] = x; q[1] = y;
    q[2] = cosf(angle); q[3] = sinf(angle);
    q[4] = -sinf(angle); q[5] = cosf(angle);
    q[6] = hx; q[7] = hy;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 300;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (steps < 0) { fprintf(stderr, "usage: place [steps >= 0]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 500.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    const float slot_x = 0.0f, slot_y = 42.0f, hx = 6.0f, hy = 5.0f;
    int spawned = 0, refused = 0;
    for (int s = 0; s < steps; ++s) {
        /* is the slot free for the next box?  (its angle changes from box to box: an AABB would over-report) */
        const float angle = 0.2f * (float)(spawned % 4);
        float slot[8];
        box_at(slot_x, slot_y, angle, hx, hy, slot);
        int32_t offsets[2], hits[8];
        int64_t total = 0;
        const int st = phx_world_query_boxes(world, slot, 1, 0, offsets, hits, 8, &total);
        if (st != PHX_ERR_CAPACITY) TRY(st);                                 /* (more than 8 bodies in the slot: occupied all the same) */
        if (total == 0) {
            const float row[5] = { slot_x, slot_y, angle, hx, hy };
            int32_t first = -1;
            TRY(phx_world_add_bodies(world, row, 1, &first));
            ++spawned;
            /* the check: the slot now holds the new body and nothing else */
            TRY(phx_world_query_boxes(world, slot, 1, 0, offsets, hits, 8, &total));
            if (total != 1 || hits[0] != first) { fprintf(stderr, "step %d: body %d was spawned into an occupied slot (%lld bodies)\n", s, first, (long long)total); return 1; }
            printf("step %d: the slot is free: body %d spawned\n", s, first);
        } else
            ++refused;
        TRY(phx_world_update(world, dt, &cfg));
    }

    /* drop one box from high above the pile: how far can it fall? */
    float cast[11];
    box_at(slot_x, 400.0f, 0.0f, hx, hy, cast);
    cast[8] = 0.0f; cast[9] = -1.0f; cast[10] = 1000.0f;
    phx_shape_hit hit;
    TRY(phx_world_cast_boxes(world, cast, 1, 0, &hit));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("place: %d bodies spawned, %d requests refused (the slot was occupied)\n", spawned, refused);
    printf("a box dropped from y = 400 touches body %d after t = %.3f, normal (%.3f, %.3f)\n", hit.body, hit.t, hit.normal.x, hit.normal.y);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps\n", nb, nm, ncp, nj, steps);
    phx_world_destroy(world);
    return nb == spawned + 1 ? 0 : 1;
}
