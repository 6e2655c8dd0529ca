/*
 * emitter.c — a world that streams bodies, through the C ABI: every N steps an emitter drops a row of boxes onto a static shelf, and
 * a kill plane below the shelf's ends removes whatever falls off.  Bodies are spawned with phx_world_add_bodies and removed with
 * phx_world_remove_outside between steps, both on the device; the shelf is made static with phx_world_set_inverse_masses.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/emitter.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o emitter
 *   ./emitter [steps] [every] [row]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure.
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

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const int every = argc > 2 ? atoi(argv[2]) : 20;
    const int row = argc > 3 ? atoi(argv[3]) : 16;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (steps < 0 || every < 1 || row < 1 || row > 4096) { fprintf(stderr, "usage: emitter [steps >= 0] [every >= 1] [row in 1..4096]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    /* rows of `row` boxes 12 apart; the shelf, one wide box spawned and then made static (invMass = invInertia = 0), holds all but the
     * outer three or so on either side */
    const float half_row = 6.0f * (float)row, shelf_half = half_row > 60.0f ? half_row - 36.0f : 24.0f;
    const float shelf[5] = { 0.0f, 0.0f, 0.0f, shelf_half, 10.0f };
    int32_t first = -1;
    TRY(phx_world_add_bodies(world, shelf, 1, &first));
    const int32_t shelf_index[1] = { first };
    const float shelf_static[2] = { 0.0f, 0.0f };
    TRY(phx_world_set_inverse_masses(world, shelf_index, shelf_static, 1));

    /* the kill plane: every body whose AABB leaves this box goes */
    const float keep[4] = { -half_row - 1000.0f, -200.0f, half_row + 1000.0f, 2000.0f };
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    float* spawn = (float*)malloc(sizeof(float) * 5 * (size_t)row);
    if (!spawn) { fprintf(stderr, "out of memory\n"); return 1; }
    long long spawned = 1, removed = 0;
    for (int s = 0; s < steps; ++s) {
        if (s % every == 0) {
            /* a row above the shelf, a little wider than it: the outer boxes fall past its ends */
            for (int k = 0; k < row; ++k) {
                float* q = spawn + 5 * k;
                q[0] = -half_row + 12.0f * ((float)k + 0.5f) + (float)(s % 7);
                q[1] = 300.0f;
                q[2] = 0.05f * (float)((s / every + k) % 5 - 2);
                q[3] = 5.0f; q[4] = 5.0f;
            }
            TRY(phx_world_add_bodies(world, spawn, row, &first));
            spawned += row;
        }
        int32_t gone = 0;
        TRY(phx_world_remove_outside(world, keep, &gone, NULL));
        removed += gone;
        TRY(phx_world_update(world, dt, &cfg));
    }
    TRY(phx_world_synchronize(world));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("emitter: %lld bodies spawned, %lld removed below the kill plane\n", spawned, removed);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps\n", nb, nm, ncp, nj, steps);
    free(spawn);
    phx_world_destroy(world);
    return nb == (int32_t)(spawned - removed) ? 0 : 1;
}
