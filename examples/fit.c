/*
 * fit.c — the marble emitter that looks first, through the C ABI: examples/place.c's loop in its round form.  Every frame it asks
 * phx_world_query_circles whether the slot above examples/marbles.c's funnel is free for the next marble and spawns it only then, so no
 * marble is ever created inside another one.  A query circle is exact against discs and boxes alike: a marble beside the slot whose
 * frame square reaches into it does not block the spawn.  At the end one marble is dropped straight down through the funnel's gap with
 * phx_world_cast_circles, which says how far it can fall before it touches the pile in the tray.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/fit.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o fit
 *   ./fit [steps] [dump]
 *
 * `dump`, if given, receives the world the cast saw: an int32 body count, the phx_rigid_body records, the phx_shape records (the tests
 * hold the printed answer to the specification on them).
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

/* one circle {px, py, angle, r}: phyx_amd.World.add_circles for one body (examples/marbles.c has the batched form) */
static int add_circle(phx_world* world, float x, float y, float angle, float r, int32_t* body)
{
    const float row[5] = { x, y, angle, r, r };
    const phx_shape shape = { PHX_SHAPE_CIRCLE, r, r };
    const float mass = 1e-5f * 0.785398f * r * r, inertia = mass * 1.5f * r * r;          /* include/phyx_amd.h SHAPES */
    const float inverse[2] = { 1.0f / mass, 1.0f / inertia };
    int st = phx_world_add_bodies(world, row, 1, body);
    if (st == PHX_OK) st = phx_world_set_shapes(world, body, &shape, 1);
    if (st == PHX_OK) st = phx_world_set_inverse_masses(world, body, inverse, 1);
    return st;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const char* dump = argc > 2 ? argv[2] : NULL;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (steps < 0) { fprintf(stderr, "usage: fit [steps >= 0] [dump]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    /* the tray and the funnel of examples/marbles.c (a gap of 24 between the walls' lower ends): static boxes */
    const int32_t floor_ = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 70.0f, 2.0f);
    const int32_t left = phx_world_add_body(world, -68.0f, 14.0f, 0.0f, 2.0f, 12.0f);
    const int32_t right = phx_world_add_body(world, 68.0f, 14.0f, 0.0f, 2.0f, 12.0f);
    const int32_t wall1 = phx_world_add_body(world, -31.0f, 66.0f, -0.7f, 25.0f, 1.5f);
    const int32_t wall2 = phx_world_add_body(world, 31.0f, 66.0f, 0.7f, 25.0f, 1.5f);
    if (floor_ < 0 || left < 0 || right < 0 || wall1 < 0 || wall2 < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int32_t statics[5] = { floor_, left, right, wall1, wall2 };
    for (int k = 0; k < 5; ++k) TRY(phx_world_set_body_static(world, statics[k]));

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    const float slot_x = -24.0f, slot_y = 100.0f;
    int spawned = 0, refused = 0;
    for (int s = 0; s < steps; ++s) {
        /* is the slot free for the next marble?  (radii 2 and 3 in turn) */
        const float r = spawned % 2 ? 3.0f : 2.0f;
        const float slot[3] = { slot_x, slot_y, r };
        int32_t offsets[2], hits[8];
        int64_t total = 0;
        const int st = phx_world_query_circles(world, slot, 1, 0, offsets, hits, 8, &total);
        if (st != PHX_ERR_CAPACITY) TRY(st);                                 /* (more than 8 bodies in the slot: occupied all the same) */
        if (total == 0) {
            int32_t body = -1;
            TRY(add_circle(world, slot_x, slot_y, 0.1f * (float)spawned, r, &body));
            ++spawned;
            /* the check: the slot now holds the new marble and nothing else */
            TRY(phx_world_query_circles(world, slot, 1, 0, offsets, hits, 8, &total));
            if (total != 1 || hits[0] != body) { fprintf(stderr, "step %d: body %d was spawned into an occupied slot (%lld bodies)\n", s, body, (long long)total); return 1; }
            printf("step %d: the slot is free: marble %d spawned\n", s, body);
        } else
            ++refused;
        TRY(phx_world_update(world, dt, &cfg));
    }

    /* drop one marble from high above the funnel's gap: how far can it fall? */
    const float cast[6] = { 0.0f, 200.0f, 3.0f, 0.0f, -1.0f, 1000.0f };
    phx_shape_hit hit;
    TRY(phx_world_cast_circles(world, cast, 1, 0, &hit));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    if (dump) {
        phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
        phx_shape* shapes = (phx_shape*)malloc((size_t)nb * sizeof *shapes);
        if (!bodies || !shapes) return 1;
        TRY(phx_world_get_bodies(world, bodies, nb));
        TRY(phx_world_get_shapes(world, shapes, nb));
        FILE* f = fopen(dump, "wb");
        if (!f || fwrite(&nb, sizeof nb, 1, f) != 1 || fwrite(bodies, sizeof *bodies, (size_t)nb, f) != (size_t)nb ||
            fwrite(shapes, sizeof *shapes, (size_t)nb, f) != (size_t)nb || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", dump); return 1; }
        free(bodies); free(shapes);
    }
    printf("fit: %d marbles spawned, %d requests refused (the slot was occupied)\n", spawned, refused);
    printf("a marble of radius 3 dropped from y = 200 touches body %d after t = %.9g, normal (%.9g, %.9g)\n", hit.body, hit.t, hit.normal.x, hit.normal.y);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps\n", nb, nm, ncp, nj, steps);
    phx_world_destroy(world);
    return nb == spawned + 5 ? 0 : 1;
}
