/*
 * piston.c — slider joints from plain C (include/phyx_amd.h SLIDERS): the fourth of the usual 2D joint set, solved in the pin pass.
 *   a crank-slider: a wheel pinned to the world and driven by an angle motor, a connecting rod pinned to the wheel 3 off its axle, a
 *                   piston pinned to the rod's other end and held on a horizontal world rail by a slider, kept level by an angle lock.
 *                   The piston's stroke is twice the crank radius.
 *   an elevator:    a platform on a vertical world rail with limits [0, 20] and a motor whose speed the loop reverses half way with
 *                   phx_world_set_slider_motors, which keeps the schedule.  It stops at its stops.
 *   a suspension:   a box on a vertical world rail with a spring (lower == upper, hertz > 0): it sags by g / (2 pi hertz)^2 and rests.
 * The bodies are small and the anchors lie outside them (an anchor is a point of the body's frame, not of its box), so nothing touches.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/piston.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o piston
 *   ./piston [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (the piston left its line or missed its
 * stroke, the elevator went through a stop, the spring did not settle, a schedule that was rebuilt).
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

#define RADIUS 3.0f
#define ROD 14.0f
#define TOP 20.0f
#define LIFT 15.0f
#define HERTZ 2.0f

/* s of SLIDERS for a slider against the world whose anchor1 is the carriage's centre: n . (pos - anchor2), n = axis / |axis| */
static float translation(const phx_rigid_body* carriage, const phx_slider* s)
{
    const float len = sqrtf(s->axis.x * s->axis.x + s->axis.y * s->axis.y);
    return (s->axis.x / len) * (carriage->pos.x - s->anchor2.x) + (s->axis.y / len) * (carriage->pos.y - s->anchor2.y);
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int32_t wheel = phx_world_add_body(world, 0.0f, 100.0f, 0.0f, 1.0f, 1.0f);
    const int32_t rod = phx_world_add_body(world, RADIUS + ROD / 2.0f, 100.0f, 0.0f, 2.0f, 0.3f);
    const int32_t piston = phx_world_add_body(world, RADIUS + ROD, 100.0f, 0.0f, 1.0f, 1.0f);
    const int32_t platform = phx_world_add_body(world, 100.0f, 50.0f, 0.0f, 3.0f, 1.0f);
    const int32_t box = phx_world_add_body(world, 200.0f, 50.0f, 0.0f, 2.0f, 2.0f);
    if (wheel < 0 || rod < 0 || piston < 0 || platform < 0 || box < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }

    /* the pins: the wheel's axle, the crank pin, the wrist pin */
    const phx_pin pins[3] = {
        { wheel, -1, { 0.0f, 0.0f }, { 0.0f, 100.0f }, { 0.0f, 0.0f } },
        { rod, wheel, { -ROD / 2.0f, 0.0f }, { RADIUS, 0.0f }, { 0.0f, 0.0f } },
        { piston, rod, { 0.0f, 0.0f }, { ROD / 2.0f, 0.0f }, { 0.0f, 0.0f } },
    };
    TRY(phx_world_add_pins(world, pins, 3, NULL));
    /* the angles: the wheel's motor (against the world the world is body2: a motor_speed of -2 turns the wheel with w = +2), the
       piston's lock */
    const phx_angle angles[2] = {
        { wheel, -1, -1000.0f, 1000.0f, 0.0f, 0.0f, -2.0f, 1.0f, 0.0f, 0.0f },
        { piston, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f },
    };
    TRY(phx_world_add_angles(world, angles, 2, NULL));
    /* the sliders.  body1 is the carriage, body2 the rail (-1: the world, anchor2 a world point, the axis in world coordinates).  The
       kind of the row along the rail follows from the data: lower < upper are limits, lower == upper a lock, with hertz > 0 a spring;
       max_force > 0 a motor */
    const phx_slider sliders[3] = {
        { piston, -1, { 0.0f, 0.0f }, { 0.0f, 100.0f }, { 1.0f, 0.0f }, -100.0f, 100.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0 },
        { platform, -1, { 0.0f, 0.0f }, { 100.0f, 50.0f }, { 0.0f, 1.0f }, 0.0f, TOP, 0.0f, 0.0f, LIFT, 1.0f, 0.0f, 0.0f, 0.0f, 0 },
        { box, -1, { 0.0f, 0.0f }, { 200.0f, 50.0f }, { 0.0f, 1.0f }, 0.0f, 0.0f, HERTZ, 0.7f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0 },
    };
    int32_t first = -1;
    TRY(phx_world_add_sliders(world, sliders, 3, &first));
    TRY(phx_world_set_pin_iterations(world, 16));
    const int32_t lift = first + 1;

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    if (!bodies) return 1;
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    float lo = 1e30f, hi = -1e30f, off = 0.0f, lift_hi = -1e30f, lift_lo = 1e30f, lift_half = 0.0f;
    for (int s = 0; s < steps; ++s) {
        if (s == steps / 2) {
            const float down[2] = { -LIFT, 1.0f };
            TRY(phx_world_set_slider_motors(world, &lift, down, 1));
        }
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_bodies(world, bodies, nb));
        const float x = translation(&bodies[piston], &sliders[0]), y = fabsf(bodies[piston].pos.y - 100.0f), e = translation(&bodies[platform], &sliders[1]);
        if (x < lo) lo = x;
        if (x > hi) hi = x;
        if (y > off) off = y;
        if (e > lift_hi) lift_hi = e;
        if (e < lift_lo) lift_lo = e;
        if (s == steps / 2 - 1) lift_half = e;
    }
    phx_slider got[3];
    int32_t ns = 0;
    TRY(phx_world_slider_count(world, &ns));
    if (ns != 3) { fprintf(stderr, "%d sliders\n", ns); return 1; }
    TRY(phx_world_get_sliders(world, got, ns));
    int64_t builds = 0;
    TRY(phx_world_pin_schedule_builds(world, &builds));
    const float lift_end = translation(&bodies[platform], &sliders[1]), sag = translation(&bodies[box], &sliders[2]);
    const float omega = 6.2831855f * HERTZ, rest = gravity / (omega * omega);
    printf("piston: %d sliders after %d steps; the piston ran from %.5f to %.5f, a stroke of %.5f (crank radius %.1f), and left its line by %.6f at the most\n",
           ns, steps, lo, hi, hi - lo, RADIUS, off);
    printf("elevator: between %.5f and %.5f (stops 0 and %.0f), at %.5f before the reversal and at %.5f at the end, stop impulse %.6f\n", lift_lo, lift_hi,
           TOP, lift_half, lift_end, got[1].axis_impulse);
    printf("suspension: sags %.5f (g / w^2 = %.5f), spring impulse %.6f; the schedule was built %lld time(s)\n", sag, rest, got[2].axis_impulse, (long long)builds);
    free(bodies);
    phx_world_destroy(world);
    if (!(off < 0.01f)) { fprintf(stderr, "the piston left its line\n"); return 1; }
    if (steps >= 200 && !(fabsf((hi - lo) - 2.0f * RADIUS) < 0.1f)) { fprintf(stderr, "the piston missed its stroke\n"); return 1; }
    /* a limit engages the step after the carriage passes it: one step's travel of slack */
    if (!(lift_hi < TOP + LIFT * dt + 0.01f) || !(lift_lo > -LIFT * dt - 0.01f)) { fprintf(stderr, "the elevator went through a stop\n"); return 1; }
    if (steps >= 400 && (!(fabsf(lift_half - TOP) < 0.05f) || !(fabsf(lift_end) < 0.05f))) { fprintf(stderr, "the elevator is not at its stop\n"); return 1; }
    if (steps >= 300 && !(fabsf(sag - rest) < 0.01f)) { fprintf(stderr, "the spring did not settle\n"); return 1; }
    if (builds != 1) { fprintf(stderr, "an edit rebuilt the schedule\n"); return 1; }
    return 0;
}
