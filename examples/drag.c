/*
 * drag.c — the reference's demo loop, headless, through the C ABI (ref: src/main.cpp:337-349): before every World::Update the
 * application reads body 1 and drags it toward a target with `acceleration.y -= gravity; acceleration += (dstVelocity - velocity) * 5`.
 * Here the target moves at a bounded speed from body 1's start, down and through a small stack, and then stays put.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/drag.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o drag
 *   ./drag [steps]
 *
 * Per step the host reads one 128-byte record (phx_world_get_body_states) and queues one 12-byte edit (phx_world_add_accelerations);
 * the step itself runs on the device.  Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure.
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

/* the target after `step` steps at `speed` units per step along the polyline px / py (n points) */
static void target_at(int step, float speed, const float* px, const float* py, int n, float* tx, float* ty)
{
    float left = speed * (float)step;
    for (int k = 0; k + 1 < n; ++k) {
        const float dx = px[k + 1] - px[k], dy = py[k + 1] - py[k], d = sqrtf(dx * dx + dy * dy);
        if (left <= d) { *tx = px[k] + dx * (left / d); *ty = py[k] + dy * (left / d); return; }
        left -= d;
    }
    *tx = px[n - 1]; *ty = py[n - 1];
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 240;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    /* ref: main.cpp:88-95: the ground and the 30 x 30 box at (-1000, 1500) that the mouse drags; then a small stack */
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 10000.0f, 10.0f);
    const int dragged = phx_world_add_body(world, -1000.0f, 1500.0f, 0.0f, 30.0f, 30.0f);
    if (ground != 0 || dragged != 1) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 8; ++r)
            if (phx_world_add_body(world, 12.0f * (float)c - 30.0f, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }

    const float px[] = {-1000.0f, -150.0f, -150.0f, 200.0f}, py[] = {1500.0f, 200.0f, 45.0f, 45.0f};
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };      /* ref: main.cpp:348 */
    const int32_t which[1] = { dragged };
    phx_rigid_body b;
    TRY(phx_world_get_body_states(world, which, 1, &b));
    const float x0 = b.pos.x, y0 = b.pos.y;
    float tx = x0, ty = y0;
    for (int s = 0; s < steps; ++s) {
        TRY(phx_world_get_body_states(world, which, 1, &b));                 /* RigidBody* draggedBody = &world.bodies[1] */
        target_at(s, 12.0f, px, py, 4, &tx, &ty);
        const float dst_x = (tx - b.pos.x) * 5e1f, dst_y = (ty - b.pos.y) * 5e1f;
        float accel[3] = { 0.0f, 0.0f, 0.0f };
        accel[1] -= gravity;                                                 /* draggedBody->acceleration.y -= gravity */
        accel[0] += (dst_x - b.velocity.x) * 5.0f;                           /* draggedBody->acceleration += (dstVelocity - velocity) * 5 */
        accel[1] += (dst_y - b.velocity.y) * 5.0f;
        TRY(phx_world_add_accelerations(world, which, accel, 1));
        TRY(phx_world_update(world, dt, &cfg));
    }
    TRY(phx_world_get_body_states(world, which, 1, &b));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("body 1: start (%.3f, %.3f) end (%.3f, %.3f) target (%.3f, %.3f)\n", x0, y0, b.pos.x, b.pos.y, tx, ty);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps\n", nb, nm, ncp, nj, steps);
    phx_world_destroy(world);
    return 0;
}
