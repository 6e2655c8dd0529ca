/*
 * bullet.c — continuous bodies from plain C (include/phyx_amd.h CONTINUOUS BODIES, phx_world_set_continuous).
 *   the scene:  a thin static wall (half a unit thick) and ramp.c's static wedge, whose foot thins out to nothing.
 *   fired:      a row of eight marbles of radius 0.25 at the wall and eight square onto the slope above the wedge's thin foot, all at
 *               120 units/s: 2 units per step at 60 Hz, eight times their radius.  (The marbles share a negative collision group: they
 *               are bullets, not a pile.)
 * The scene is run twice.  Discrete, IntegratePosition moves a marble in one jump and the broadphase sees only where it lands: the
 * marbles pass the wall and the foot without one manifold ever existing.  Continuous (one call: phx_world_set_continuous with a core
 * radius of 0.8 of the marble's), each marble's core disc is swept along the step's translation and the marble is put back to just short
 * of the first touch (a 64th of the core radius: the header's skin); the next step's ordinary contact stops it.  The example prints how many marbles ended beyond the wall and beyond the
 * wedge in each run, and the sweep hits of the first continuous step (phx_world_sweep_hits): the wedge's are on its slope, with the
 * slope's normal, not on its frame box.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/bullet.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o bullet
 *   ./bullet [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a continuous marble that tunnelled, a discrete
 * one that did not pass the wall).
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

#define ROW 8
#define MARBLES (2 * ROW)

static const float R = 0.25f, SPEED = 120.0f, DT = 1.0f / 60.0f;

/* one run of the scene: *past_wall and *past_wedge receive how many marbles ended beyond each obstacle */
static int run(int continuous, int steps, int* past_wall, int* past_wedge)
{
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    /* body 0: the wall, x in [-0.25, 0.25]; body 1: ramp.c's wedge at (60, 0): its face runs from (30, 22) down to (90, -8) */
    const float wall[5] = { 0.0f, 0.0f, 0.0f, 0.25f, 12.0f }, frame[5] = { 60.0f, 0.0f, 0.0f, 30.0f, 22.0f }, none[4] = { 0.f, 0.f, 0.f, 0.f };
    const phx_polygon wedge = { 3, { { -30.f, -8.f }, { 30.f, -8.f }, { -30.f, 22.f } } };
    const int32_t statics[2] = { 0, 1 }, second = 1;
    int32_t first = -1;
    TRY(phx_world_add_bodies(world, wall, 1, &first));
    TRY(phx_world_add_bodies(world, frame, 1, &first));
    TRY(phx_world_set_polygons(world, &second, &wedge, 1));
    TRY(phx_world_set_inverse_masses(world, statics, none, 2));

    /* the marbles: bodies 2 .. 9 in front of the wall, flying right; bodies 10 .. 17 half a unit off the slope above the wedge's foot (the
     * wedge is 1 to 0.125 units thick there), flying along -n, n = (1, 2) / sqrt(5) the slope's normal */
    const float nx = 0.4472136f, ny = 0.8944272f;
    float rows[MARBLES][5], masses[MARBLES][2], velocities[MARBLES][3], radii[MARBLES];
    phx_collision_filter filters[MARBLES];
    phx_shape circles[MARBLES];
    int32_t marbles[MARBLES];
    const float mass = 1e-5f * 0.785398f * R * R;
    for (int k = 0; k < MARBLES; ++k) {
        const int down = k >= ROW;
        const float fx = 88.0f + 0.25f * (float)(k - ROW), fy = 7.0f - 0.5f * (fx - 60.0f);      /* a point of the slope */
        const float x = down ? fx + 0.5f * nx : -1.0f, y = down ? fy + 0.5f * ny : -7.0f + 2.0f * (float)k;
        const float row[5] = { x, y, 0.f, R, R }, v[3] = { down ? -SPEED * nx : SPEED, down ? -SPEED * ny : 0.f, 0.f };
        for (int c = 0; c < 5; ++c) rows[k][c] = row[c];
        for (int c = 0; c < 3; ++c) velocities[k][c] = v[c];
        masses[k][0] = 1.0f / mass; masses[k][1] = 1.0f / (mass * 1.5f * R * R);
        circles[k].kind = PHX_SHAPE_CIRCLE; circles[k].hx = R; circles[k].hy = R;
        filters[k].category = 1u; filters[k].mask = 0xFFFFFFFFu; filters[k].group = -1;
        radii[k] = 0.8f * R;                                                                 /* the core: strictly inside the marble */
        marbles[k] = 2 + k;
    }
    TRY(phx_world_add_bodies(world, &rows[0][0], MARBLES, &first));
    TRY(phx_world_set_shapes(world, marbles, circles, MARBLES));
    TRY(phx_world_set_inverse_masses(world, marbles, &masses[0][0], MARBLES));
    TRY(phx_world_set_velocities(world, marbles, &velocities[0][0], MARBLES));
    TRY(phx_world_set_collision_filters(world, marbles, filters, MARBLES, NULL));
    if (continuous) TRY(phx_world_set_continuous(world, marbles, radii, MARBLES));           /* the one call */

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    for (int s = 0; s < steps; ++s) {
        TRY(phx_world_update(world, DT, &cfg));
        if (continuous && s == 0) {
            phx_sweep_hit hits[MARBLES];
            int64_t total = 0;
            TRY(phx_world_sweep_hits(world, hits, MARBLES, &total));
            printf("sweep: %lld hits in the first continuous step\n", (long long)total);
            for (int64_t k = 0; k < total; ++k)
                printf("  body %d stopped by body %d at t = %.4f, normal (%.4f, %.4f)\n", hits[k].body, hits[k].target, hits[k].t, hits[k].normal.x, hits[k].normal.y);
        }
    }
    phx_rigid_body bodies[2 + MARBLES];
    TRY(phx_world_get_bodies(world, bodies, 2 + MARBLES));
    *past_wall = 0; *past_wedge = 0;
    for (int k = 0; k < ROW; ++k) *past_wall += bodies[2 + k].pos.x > 0.25f + R;
    for (int k = ROW; k < MARBLES; ++k) *past_wedge += bodies[2 + k].pos.y < -8.0f - R;
    int64_t passes = 0, clamps = 0;
    TRY(phx_world_sweep_counts(world, &passes, &clamps));
    printf("bullet: %s: %d of %d beyond the wall, %d of %d beyond the wedge after %d steps; %lld passes, %lld clamps\n", continuous ? "continuous" : "discrete",
           *past_wall, ROW, *past_wedge, ROW, steps, (long long)passes, (long long)clamps);
    phx_world_destroy(world);
    return 0;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 30;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    int wall[2] = { 0, 0 }, wedge[2] = { 0, 0 };
    for (int continuous = 0; continuous < 2; ++continuous) {
        const int st = run(continuous, steps, &wall[continuous], &wedge[continuous]);
        if (st) return st;
    }
    if (wall[0] != ROW) { fprintf(stderr, "%d of %d discrete marbles passed the wall\n", wall[0], ROW); return 1; }
    if (wall[1] || wedge[1]) { fprintf(stderr, "%d continuous marbles tunnelled\n", wall[1] + wedge[1]); return 1; }
    return 0;
}
