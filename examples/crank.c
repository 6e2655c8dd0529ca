/*
 * crank.c — angle joints from plain C (include/phyx_amd.h ANGLES): the third of the usual 2D joint set, solved in the pin pass.
 *   a door:   a tall box pinned to the world at its foot, limited to +-0.5 rad against the world.  It leans, tips over, a box falls on
 *             it, and it stops at its stop.
 *   a wheel:  pinned to a static chassis and driven by a motor (a range far wider than a turn: no limits) whose speed the loop
 *             reverses half way with phx_world_set_angle_motors, which keeps the schedule.
 *   a weld:   two boxes joined by a pin plus a lock at 0, hung from the world by a second pin: they swing as one body.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/crank.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o crank
 *   ./crank [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (the door went through its stop, the wheel
 * missed its speed, the weld bent, a schedule that was rebuilt).
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

#define STOP 0.5f
#define SPEED 4.0f

/* theta of ANGLES: the clockwise angle of b's frame against a's (b = NULL: the world) */
static float theta(const phx_rigid_body* a, const phx_rigid_body* b)
{
    const float bx = b ? b->xvector.x : 1.0f, by = b ? b->xvector.y : 0.0f;
    const float c = a->xvector.x * bx + a->xvector.y * by, s = a->xvector.x * by - a->xvector.y * bx;
    return (float)atan2((double)-s, (double)c);
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int32_t ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 60.0f, 2.0f);
    const int32_t door = phx_world_add_body(world, -0.9f, 19.9f, 0.15f, 1.0f, 6.0f);
    const int32_t pusher = phx_world_add_body(world, -3.5f, 36.0f, 0.0f, 2.0f, 2.0f);
    const int32_t chassis = phx_world_add_body(world, 100.0f, 40.0f, 0.0f, 6.0f, 1.0f);
    const int32_t wheel = phx_world_add_body(world, 100.0f, 34.0f, 0.0f, 2.0f, 2.0f);
    const int32_t arm = phx_world_add_body(world, 205.0f, 60.0f, 0.0f, 5.0f, 1.0f);
    const int32_t hand = phx_world_add_body(world, 215.0f, 60.0f, 0.0f, 5.0f, 1.0f);
    if (ground < 0 || door < 0 || pusher < 0 || chassis < 0 || wheel < 0 || arm < 0 || hand < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    TRY(phx_world_set_body_static(world, chassis));

    /* the pins: the door's foot, the wheel's axle (below the chassis, so that the two do not touch), the weld's joint, its hook */
    const phx_pin pins[4] = {
        { door, -1, { 0.0f, -6.0f }, { 0.0f, 14.0f }, { 0.0f, 0.0f } },
        { wheel, chassis, { 0.0f, 0.0f }, { 0.0f, -6.0f }, { 0.0f, 0.0f } },
        { hand, arm, { -5.0f, 0.0f }, { 5.0f, 0.0f }, { 0.0f, 0.0f } },
        { arm, -1, { -5.0f, 0.0f }, { 200.0f, 60.0f }, { 0.0f, 0.0f } },
    };
    TRY(phx_world_add_pins(world, pins, 4, NULL));

    /* the angles.  The kind follows from the data: lower < upper are limits, lower == upper a lock, max_torque > 0 a motor; theta is
       the clockwise angle of body2 against body1 and the motor drives w(body2) - w(body1), so the wheel is body2 */
    const phx_angle angles[3] = {
        { door, -1, -STOP, STOP, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f },
        { chassis, wheel, -1000.0f, 1000.0f, 0.0f, 0.0f, SPEED, 0.05f, 0.0f, 0.0f },
        { arm, hand, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f },
    };
    int32_t first = -1;
    TRY(phx_world_add_angles(world, angles, 3, &first));
    TRY(phx_world_set_pin_iterations(world, 16));
    const int32_t motor = first + 1;

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    if (!bodies) return 1;
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    float door_worst = 0.0f, weld_worst = 0.0f, swing = 0.0f, wheel_first = 0.0f;
    for (int s = 0; s < steps; ++s) {
        if (s == steps / 2) {
            const float reverse[2] = { -SPEED, 0.05f };
            TRY(phx_world_set_angle_motors(world, &motor, reverse, 1));
        }
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_bodies(world, bodies, nb));
        const float d = fabsf(theta(&bodies[door], NULL)), w = fabsf(theta(&bodies[arm], &bodies[hand])), a = fabsf(theta(&bodies[arm], NULL));
        if (d > door_worst) door_worst = d;
        if (w > weld_worst) weld_worst = w;
        if (a > swing) swing = a;
        if (s == steps / 2 - 1) wheel_first = bodies[wheel].angular_velocity;
    }
    phx_angle got[3];
    int32_t na = 0;
    TRY(phx_world_angle_count(world, &na));
    if (na != 3) { fprintf(stderr, "%d angles\n", na); return 1; }
    TRY(phx_world_get_angles(world, got, na));
    int64_t builds = 0;
    TRY(phx_world_pin_schedule_builds(world, &builds));
    const float door_end = theta(&bodies[door], NULL), wheel_end = bodies[wheel].angular_velocity;
    printf("crank: %d angles after %d steps; the door went to %.4f at the most and stands at %.4f (stop %.1f), impulse %.6f\n", na, steps, door_worst,
           door_end, STOP, got[0].impulse);
    printf("wheel: %.4f rad/s before the reversal, %.4f after; weld: bent %.5f at the most while it swung %.3f; the schedule was built %lld time(s)\n",
           wheel_first, wheel_end, weld_worst, swing, (long long)builds);
    free(bodies);
    phx_world_destroy(world);
    /* a limit engages the step after the angle passes it and takes a fifth of the error back per step: one step's travel of slack */
    if (!(door_worst < STOP + 0.1f) || !(fabsf(fabsf(door_end) - STOP) < 0.02f)) { fprintf(stderr, "the door is not at its stop\n"); return 1; }
    if (!(fabsf(wheel_first - SPEED) < 0.01f) || !(fabsf(wheel_end + SPEED) < 0.01f)) { fprintf(stderr, "the wheel missed its speed\n"); return 1; }
    if (!(weld_worst < 0.02f) || !(swing > 0.5f)) { fprintf(stderr, "the weld bent, or never swung\n"); return 1; }
    if (builds != 1) { fprintf(stderr, "an edit rebuilt the schedule\n"); return 1; }
    return 0;
}
