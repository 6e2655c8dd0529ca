/*
 * layers.c — collision filters in a demo loop: a stack of boxes on the ground, and a row of ghosts dropped onto it.  The ghosts are a
 * layer of their own (category 2) that only collides with the ground (category 4): they fall through the stack and come to rest on
 * the ground, inside its bottom row.  Half way through, one phx_world_set_collision_filters call gives them the default filter back:
 * they are solid again, and the solver pushes them out of the boxes they overlap.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/layers.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o layers
 *   ./layers [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or the ghosts did not behave as described).
 */
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

#define COLUMNS 5
#define ROWS 6
#define GHOSTS COLUMNS
#define MAX_BODIES (1 + COLUMNS * ROWS + GHOSTS)
#define MAX_MANIFOLDS 4096

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 240;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    if (steps < 60) { fprintf(stderr, "usage: layers [steps >= 60]\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 1000.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int c = 0; c < COLUMNS; ++c)
        for (int r = 0; r < ROWS; ++r)
            if (phx_world_add_body(world, 12.0f * (float)c - 24.0f, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int first_ghost = 1 + COLUMNS * ROWS;
    int32_t ghosts[GHOSTS];
    for (int g = 0; g < GHOSTS; ++g) {
        ghosts[g] = phx_world_add_body(world, 12.0f * (float)g - 22.0f, 200.0f, 0.0f, 4.0f, 4.0f);
        if (ghosts[g] != first_ghost + g) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    }

    /* the layers: the ground is category 4 and collides with everything; the stack keeps the default {1, all, 0}; the ghosts are
     * category 2 and collide only with category 4 */
    const int32_t ground_list[1] = { ground };
    const phx_collision_filter ground_filter = { 4u, 0xFFFFFFFFu, 0 };
    phx_collision_filter ghost_filters[GHOSTS], solid[GHOSTS];
    for (int g = 0; g < GHOSTS; ++g) {
        ghost_filters[g] = (phx_collision_filter){ 2u, 4u, 0 };
        solid[g] = (phx_collision_filter){ 1u, 0xFFFFFFFFu, 0 };
    }
    TRY(phx_world_set_collision_filters(world, ground_list, &ground_filter, 1, NULL));
    TRY(phx_world_set_collision_filters(world, ghosts, ghost_filters, GHOSTS, NULL));

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    static float poses[4 * MAX_BODIES];
    static phx_manifold manifolds[MAX_MANIFOLDS];
    int fell = 0, solid_pairs = 0;
    for (int s = 0; s < steps; ++s) {
        if (s == steps / 2) {
            /* the ghosts should lie on the ground, inside the bottom row of the stack */
            TRY(phx_world_get_poses(world, poses, MAX_BODIES));
            float lowest = 1e30f, highest = -1e30f;
            for (int g = 0; g < GHOSTS; ++g) {
                const float y = poses[4 * ghosts[g] + 1];
                lowest = y < lowest ? y : lowest;
                highest = y > highest ? y : highest;
            }
            fell = highest < 20.0f && lowest > 10.0f;
            printf("step %3d: ghost layer below the stack: ghost centres at y %.2f .. %.2f (the ground's top is y 10)\n", s, lowest, highest);
            int32_t dropped = 0;
            TRY(phx_world_set_collision_filters(world, ghosts, solid, GHOSTS, &dropped));      /* one call: solid again */
            printf("step %3d: the ghosts take the default filter (%d manifolds dropped)\n", s, dropped);
        }
        TRY(phx_world_update(world, dt, &cfg));
    }
    TRY(phx_world_synchronize(world));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    if (nm > MAX_MANIFOLDS) { fprintf(stderr, "more manifolds than the example has room for\n"); return 1; }
    TRY(phx_world_get_manifolds(world, manifolds, MAX_MANIFOLDS));
    for (int i = 0; i < nm; ++i) {
        const int g1 = manifolds[i].body1 >= first_ghost, g2 = manifolds[i].body2 >= first_ghost;
        const int s1 = manifolds[i].body1 > 0 && !g1, s2 = manifolds[i].body2 > 0 && !g2;
        solid_pairs += (g1 && s2) || (g2 && s1);
    }
    printf("solid again: %d manifolds between ghosts and stack boxes after %d steps; world: %d bodies %d manifolds %d joints\n",
           solid_pairs, steps, nb, nm, nj);
    phx_world_destroy(world);
    if (!fell) { fprintf(stderr, "the ghosts did not fall through the stack onto the ground\n"); return 1; }
    if (!solid_pairs) { fprintf(stderr, "the ghosts never touched the stack once solid\n"); return 1; }
    return 0;
}
