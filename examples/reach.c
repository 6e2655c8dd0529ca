/*
 * reach.c — pick.c's loop with a tolerant pick, through the C ABI: a cursor sweeps across examples/marbles.c's funnel while marbles
 * fall into it; phx_world_query_nearest(..., PHX_QUERY_SKIP_STATIC, ...) finds the dynamic body nearest to the cursor within 2 units
 * (the cursor need not be inside it, and the funnel's walls are never grabbed), and that body is dragged as in drag.c.  Every second
 * the clearance of each marble from the nearest static body is printed: the nearest query of the marble's centre against a second
 * world that holds the funnel alone, less the marble's radius.  A clearance below zero is a marble pressed into a wall; the program
 * fails if it sees one while the marble has no contact (phx_world_query_contacts).  The clearances are taken between
 * phx_world_pre_solve and phx_world_finish_step, of the geometry that step's narrowphase saw: a marble that lands in a step meets the
 * narrowphase in the next one.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/reach.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o reach
 *   ./reach [steps] [dump]
 *
 * `dump`, if given, receives the world the first pick saw: an int32 body count, the phx_rigid_body records, the phx_shape records (the
 * tests hold the printed pick to the specification on them).
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (nothing was ever picked, or a marble inside a
 * wall without a contact).
 */
#include <float.h>
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

#define MAX_MARBLES 64

/* the tray and the funnel of examples/marbles.c: five static boxes, bodies 0 .. 4 */
static int add_funnel(phx_world* world)
{
    const float boxes[5][5] = { { 0.0f, 0.0f, 0.0f, 70.0f, 2.0f }, { -68.0f, 14.0f, 0.0f, 2.0f, 12.0f }, { 68.0f, 14.0f, 0.0f, 2.0f, 12.0f },
                                { -31.0f, 66.0f, -0.7f, 25.0f, 1.5f }, { 31.0f, 66.0f, 0.7f, 25.0f, 1.5f } };
    for (int k = 0; k < 5; ++k) {
        const int32_t b = phx_world_add_body(world, boxes[k][0], boxes[k][1], boxes[k][2], boxes[k][3], boxes[k][4]);
        if (b != k) return PHX_ERR_STATE;
        const int st = phx_world_set_body_static(world, b);
        if (st != PHX_OK) return st;
    }
    return PHX_OK;
}

/* one circle {px, py, angle, r} (examples/fit.c) */
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

static int dump_world(phx_world* world, const char* path)
{
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    phx_shape* shapes = (phx_shape*)malloc((size_t)nb * sizeof *shapes);
    if (!bodies || !shapes) return 1;
    TRY(phx_world_get_bodies(world, bodies, nb));
    TRY(phx_world_get_shapes(world, shapes, nb));
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(&nb, sizeof nb, 1, f) != 1 || fwrite(bodies, sizeof *bodies, (size_t)nb, f) != (size_t)nb ||
        fwrite(shapes, sizeof *shapes, (size_t)nb, f) != (size_t)nb || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    free(bodies); free(shapes);
    return 0;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 360;
    const char* dump = argc > 2 ? argv[2] : NULL;
    const float gravity = -200.0f, dt = 1.0f / 60.0f, reach = 2.0f;
    if (steps < 0) { fprintf(stderr, "usage: reach [steps >= 0] [dump]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world *world = NULL, *walls = NULL;                                  /* the world, and the funnel alone: what "static" means here */
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_create(&walls, 0));
    TRY(phx_world_set_gravity(world, gravity));
    TRY(add_funnel(world));
    TRY(add_funnel(walls));

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    int32_t marbles[MAX_MARBLES], held = -1;
    float radii[MAX_MARBLES];
    int count = 0, picks = 0, inside = 0;
    for (int s = 0; s < steps; ++s) {
        /* a marble every tenth step above the left wall, radii 2 and 3 in turn, while the slot is clear of everything by its radius */
        if (s % 10 == 0 && count < MAX_MARBLES) {
            const float r = count % 2 ? 3.0f : 2.0f;
            const float slot[3] = { -24.0f, 100.0f, r };
            phx_near_hit at;
            TRY(phx_world_query_nearest(world, slot, 1, 0, &at));
            if (at.body < 0) {
                TRY(add_circle(world, slot[0], slot[1], 0.1f * (float)count, r, &marbles[count]));
                radii[count++] = r;
            }
        }
        /* the cursor sweeps the tray from left to right and back, 6 units above the floor */
        const int leg = (s / 120) % 2;
        const float along = (float)(s % 120) / 120.0f;
        const float cx = leg ? 60.0f - 120.0f * along : -60.0f + 120.0f * along, cy = 8.0f;
        if (held < 0) {                                                      /* the button is down: what is within reach of the cursor? */
            const float q[3] = { cx, cy, reach };
            phx_near_hit hit;
            TRY(phx_world_query_nearest(world, q, 1, PHX_QUERY_SKIP_STATIC, &hit));
            if (hit.body >= 0) {
                held = hit.body;
                if (picks++ == 0) {
                    printf("step %d: reached body %d at distance %.9g from (%.9g, %.9g), surface point (%.9g, %.9g)\n", s, hit.body, hit.distance, cx, cy,
                           hit.point.x, hit.point.y);
                    if (dump && dump_world(world, dump) != 0) return 1;
                }
            }
        }
        if (held >= 0) {
            phx_rigid_body b;
            TRY(phx_world_get_body_states(world, &held, 1, &b));
            float accel[3] = { 0.0f, 0.0f, 0.0f };
            accel[1] -= gravity;                                             /* drag.c: acceleration.y -= gravity; += (dstVelocity - velocity) * 5 */
            accel[0] += ((cx - b.pos.x) * 5e1f - b.velocity.x) * 5.0f;
            accel[1] += ((cy + 20.0f - b.pos.y) * 5e1f - b.velocity.y) * 5.0f;
            TRY(phx_world_add_accelerations(world, &held, accel, 1));
            if (s % 120 == 119) held = -1;                                   /* the button goes up at the end of a sweep */
        }
        if (s % 60 != 59 || count == 0) { TRY(phx_world_update(world, dt, &cfg)); continue; }
        /* every second: how close is each marble to the funnel?  The step is split at the solver boundary (pre_solve + finish_step ==
         * update): between the two a query and a gather see the geometry the step's narrowphase saw, so a marble inside a wall there
         * is one the step has made a contact for */
        phx_rigid_body states[MAX_MARBLES];
        float q[3 * MAX_MARBLES];
        phx_near_hit near_[MAX_MARBLES];
        TRY(phx_world_pre_solve(world, dt));
        TRY(phx_world_get_body_states(world, marbles, count, states));
        for (int k = 0; k < count; ++k) { q[3 * k] = states[k].pos.x; q[3 * k + 1] = states[k].pos.y; q[3 * k + 2] = FLT_MAX; }
        TRY(phx_world_query_nearest(walls, q, count, 0, near_));
        TRY(phx_world_finish_step(world, dt, &cfg));
        printf("second %d:", s / 60 + 1);
        for (int k = 0; k < count; ++k) {
            const float clearance = near_[k].distance - radii[k];
            printf(" %d:%.3f(%d)", marbles[k], clearance, near_[k].body);
            if (clearance < 0.0f) {
                int32_t offsets[2];
                phx_contact contacts[16];
                int64_t total = 0;
                const int st = phx_world_query_contacts(world, &marbles[k], 1, 0, offsets, contacts, 16, &total);
                if (st != PHX_ERR_CAPACITY) TRY(st);
                ++inside;
                if (total == 0) { fprintf(stderr, "\nmarble %d is %.3f inside body %d and has no contact\n", marbles[k], -clearance, near_[k].body); return 1; }
            }
        }
        printf("\n");
    }
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("reach: %d marbles, %d pick(s), %d clearances below zero (each with a contact)\n", count, picks, inside);
    printf("world: %d bodies %d manifolds %d contact points %d joints after %d steps\n", nb, nm, ncp, nj, steps);
    phx_world_destroy(walls);
    phx_world_destroy(world);
    if (steps >= 240 && picks == 0) { fprintf(stderr, "the cursor never came within reach of a body\n"); return 1; }
    return 0;
}
