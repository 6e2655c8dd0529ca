/*
 * pick.c — the reference's demo loop with a real pick (ref: src/main.cpp:337-349 drags a hard-coded body 1): a cursor moves along a
 * path; the dynamic body under it is found with phx_world_query_points(..., PHX_QUERY_SKIP_STATIC, ...) — the ground is never grabbed —
 * and dragged toward the cursor with `acceleration.y -= gravity; acceleration += (dstVelocity - velocity) * 5` as in drag.c.  One
 * downward ray per step from the cursor reports the surface below it.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/pick.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o pick
 *   ./pick [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or nothing was ever picked).
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

/* the cursor after `step` steps at `speed` units per step along the polyline px / py (n points) */
static void cursor_at(int step, float speed, const float* px, const float* py, int n, float* cx, float* cy)
{
    float left = speed * (float)step;
    for (int k = 0; k + 1 < n; ++k) {
        const float dx = px[k + 1] - px[k], dy = py[k + 1] - py[k], d = sqrtf(dx * dx + dy * dy);
        if (left <= d) { *cx = px[k] + dx * (left / d); *cy = py[k] + dy * (left / d); return; }
        left -= d;
    }
    *cx = px[n - 1]; *cy = py[n - 1];
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 240;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    /* the ground and a small stack of 6 x 8 boxes (drag.c's scene without the hard-coded body) */
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 10000.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 8; ++r)
            if (phx_world_add_body(world, 12.0f * (float)c - 30.0f, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }

    /* the button goes down inside the stack's first column (its fourth box); the cursor pulls up and to the right, then rests */
    const float px[] = {-30.0f, 60.0f, 120.0f, 120.0f}, py[] = {47.0f, 160.0f, 200.0f, 200.0f};
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };      /* ref: main.cpp:348 */
    int32_t held = -1, picks = 0, ground_hits = 0;
    float cx = px[0], cy = py[0];
    phx_ray_hit below = { -1, 0.0f, { 0.0f, 0.0f }, { 0.0f, 0.0f } };
    for (int s = 0; s < steps; ++s) {
        cursor_at(s, 3.0f, px, py, 4, &cx, &cy);
        const float cursor[2] = { cx, cy };
        if (held < 0) {                                                      /* the mouse button goes down: what is under the cursor? */
            TRY(phx_world_query_points(world, cursor, 1, PHX_QUERY_SKIP_STATIC, &held));
            if (held >= 0) { ++picks; printf("step %d: picked body %d at (%.2f, %.2f)\n", s, held, cx, cy); }
        }
        const float ray[5] = { cx, cy, 0.0f, -1.0f, 1.0e4f };                 /* straight down, 10 000 units */
        TRY(phx_world_raycast(world, ray, 1, 0, &below));
        if (below.body == ground) ++ground_hits;
        if (held >= 0) {
            phx_rigid_body b;
            TRY(phx_world_get_body_states(world, &held, 1, &b));
            const float dst_x = (cx - b.pos.x) * 5e1f, dst_y = (cy - b.pos.y) * 5e1f;
            float accel[3] = { 0.0f, 0.0f, 0.0f };
            accel[1] -= gravity;                                             /* draggedBody->acceleration.y -= gravity */
            accel[0] += (dst_x - b.velocity.x) * 5.0f;                       /* draggedBody->acceleration += (dstVelocity - velocity) * 5 */
            accel[1] += (dst_y - b.velocity.y) * 5.0f;
            TRY(phx_world_add_accelerations(world, &held, accel, 1));
        }
        TRY(phx_world_update(world, dt, &cfg));
    }
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("cursor (%.2f, %.2f): body %d held; below it body %d at t %.3f, point (%.3f, %.3f), normal (%.3f, %.3f)\n", cx, cy, held,
           below.body, below.t, below.point.x, below.point.y, below.normal.x, below.normal.y);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps; %d pick(s), the ground below the cursor %d times\n",
           nb, nm, ncp, nj, steps, picks, ground_hits);
    phx_world_destroy(world);
    if (steps > 0 && picks == 0) { fprintf(stderr, "the cursor never found a body\n"); return 1; }
    return 0;
}
