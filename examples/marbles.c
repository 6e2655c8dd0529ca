/*
 * marbles.c — round bodies from plain C (include/phyx_amd.h SHAPES).
 *   marbles:  36 circles of two radii dropped into a funnel of two tilted static boxes; they roll down the walls, fall through the gap
 *             and come to rest in a tray.
 *   a wheel:  a circle pinned at its centre to a static chassis and driven by an angle motor — examples/crank.c's wheel, round at last.
 * add_circles below is phyx_amd.World.add_circles in C, three calls: phx_world_add_bodies with half extents (r, r),
 * phx_world_set_shapes to make them circles, phx_world_set_inverse_masses with the circle's mass and inertia on AddBody's scale.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/marbles.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o marbles
 *   ./marbles [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a marble left the tray's world, a shape that
 * did not read back, the wheel missed its speed).
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

#define MARBLES 36
#define SPEED 4.0f

/* rows = {px, py, angle, r} per circle; *first = the index of the first new body */
static int add_circles(phx_world* world, const float* rows, int32_t count, int32_t* first)
{
    float* spawn = (float*)malloc((size_t)count * 5 * sizeof(float));
    int32_t* bodies = (int32_t*)malloc((size_t)count * sizeof(int32_t));
    phx_shape* shapes = (phx_shape*)malloc((size_t)count * sizeof(phx_shape));
    float* masses = (float*)malloc((size_t)count * 2 * sizeof(float));
    int st = spawn && bodies && shapes && masses ? PHX_OK : PHX_ERR_INVALID;
    for (int32_t k = 0; st == PHX_OK && k < count; ++k) {
        const float r = rows[4 * k + 3];
        spawn[5 * k] = rows[4 * k]; spawn[5 * k + 1] = rows[4 * k + 1]; spawn[5 * k + 2] = rows[4 * k + 2];
        spawn[5 * k + 3] = r; spawn[5 * k + 4] = r;
        shapes[k].kind = PHX_SHAPE_CIRCLE; shapes[k].hx = r; shapes[k].hy = r;
        const float mass = 1e-5f * 0.785398f * r * r, inertia = mass * 1.5f * r * r;      /* include/phyx_amd.h SHAPES */
        masses[2 * k] = 1.0f / mass; masses[2 * k + 1] = 1.0f / inertia;
    }
    if (st == PHX_OK) st = phx_world_add_bodies(world, spawn, count, first);                /* 1. boxes of half extents (r, r) */
    for (int32_t k = 0; st == PHX_OK && k < count; ++k) bodies[k] = *first + k;
    if (st == PHX_OK) st = phx_world_set_shapes(world, bodies, shapes, count);               /* 2. ... become circles */
    if (st == PHX_OK) st = phx_world_set_inverse_masses(world, bodies, masses, count);       /* 3. ... with a disc's mass */
    free(spawn); free(bodies); free(shapes); free(masses);
    return st;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    /* the tray, the funnel (a gap of 24 between the walls' lower ends) and the wheel's chassis: static boxes */
    const int32_t floor_ = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 70.0f, 2.0f);
    const int32_t left = phx_world_add_body(world, -68.0f, 14.0f, 0.0f, 2.0f, 12.0f);
    const int32_t right = phx_world_add_body(world, 68.0f, 14.0f, 0.0f, 2.0f, 12.0f);
    const int32_t wall1 = phx_world_add_body(world, -31.0f, 66.0f, -0.7f, 25.0f, 1.5f);
    const int32_t wall2 = phx_world_add_body(world, 31.0f, 66.0f, 0.7f, 25.0f, 1.5f);
    const int32_t chassis = phx_world_add_body(world, 200.0f, 40.0f, 0.0f, 6.0f, 1.0f);
    if (floor_ < 0 || left < 0 || right < 0 || wall1 < 0 || wall2 < 0 || chassis < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int32_t statics[6] = { floor_, left, right, wall1, wall2, chassis };
    for (int k = 0; k < 6; ++k) TRY(phx_world_set_body_static(world, statics[k]));

    /* the marbles, radii 2 and 3 in turn, in six rows above the funnel; then the wheel, below its chassis */
    float rows[(MARBLES + 1) * 4];
    for (int k = 0; k < MARBLES; ++k) {
        rows[4 * k] = -27.5f + 11.0f * (float)(k % 6) + ((k / 6) % 2 ? 2.0f : 0.0f);
        rows[4 * k + 1] = 100.0f + 9.0f * (float)(k / 6);
        rows[4 * k + 2] = 0.1f * (float)k;
        rows[4 * k + 3] = k % 2 ? 3.0f : 2.0f;
    }
    rows[4 * MARBLES] = 200.0f; rows[4 * MARBLES + 1] = 34.0f; rows[4 * MARBLES + 2] = 0.0f; rows[4 * MARBLES + 3] = 3.0f;
    int32_t first = -1;
    TRY(add_circles(world, rows, MARBLES + 1, &first));
    const int32_t wheel = first + MARBLES;

    /* the wheel's axle and its motor (theta is the angle of body2 against body1 and the motor drives w(body2) - w(body1)) */
    const phx_pin axle = { wheel, chassis, { 0.0f, 0.0f }, { 0.0f, -6.0f }, { 0.0f, 0.0f } };
    TRY(phx_world_add_pins(world, &axle, 1, NULL));
    const phx_angle motor = { chassis, wheel, -1000.0f, 1000.0f, 0.0f, 0.0f, SPEED, 0.2f, 0.0f, 0.0f };
    TRY(phx_world_add_angles(world, &motor, 1, NULL));
    TRY(phx_world_set_pin_iterations(world, 16));

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    phx_shape* shapes = (phx_shape*)malloc((size_t)nb * sizeof *shapes);
    if (!bodies || !shapes) return 1;
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    for (int s = 0; s < steps; ++s) TRY(phx_world_update(world, dt, &cfg));
    TRY(phx_world_get_bodies(world, bodies, nb));
    TRY(phx_world_get_shapes(world, shapes, nb));

    int resting = 0, through = 0, lost = 0, round_ = 0;
    for (int32_t b = 0; b < nb; ++b) round_ += shapes[b].kind == PHX_SHAPE_CIRCLE;
    for (int32_t b = first; b < first + MARBLES; ++b) {
        const phx_rigid_body* m = &bodies[b];
        const float speed = sqrtf(m->velocity.x * m->velocity.x + m->velocity.y * m->velocity.y);
        if (!(m->pos.y > 0.0f && m->pos.y < 400.0f && fabsf(m->pos.x) < 70.0f)) ++lost;      /* (a NaN counts as lost) */
        if (m->pos.y < 40.0f) ++through;
        if (speed < 1.0f && fabsf(m->angular_velocity) < 0.5f) ++resting;
    }
    const float wheel_speed = bodies[wheel].angular_velocity;
    printf("marbles: %d circles after %d steps; %d of %d marbles through the funnel, %d at rest, %d lost\n", round_, steps, through, MARBLES, resting, lost);
    printf("wheel: %.4f rad/s on its motor (set %.1f), its centre %.4f from the axle\n", wheel_speed, SPEED,
           hypotf(bodies[wheel].pos.x - 200.0f, bodies[wheel].pos.y - 34.0f));
    free(bodies); free(shapes);
    phx_world_destroy(world);
    if (round_ != MARBLES + 1) { fprintf(stderr, "%d circles read back, %d were made\n", round_, MARBLES + 1); return 1; }
    if (lost) { fprintf(stderr, "%d marbles left the tray\n", lost); return 1; }
    if (!(fabsf(wheel_speed - SPEED) < 0.01f)) { fprintf(stderr, "the wheel missed its speed\n"); return 1; }
    return 0;
}
