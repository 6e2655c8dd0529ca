/*
 * bridge.c — links from plain C (include/phyx_amd.h LINKS): a deck of 8 planks pinned end to end between two static posts, a rod hanger
 * from every plank to a fixed point above it, a crate on a rope below the middle of the deck (slack until the crate has fallen far
 * enough, then taut) and a box drawn by a spring towards a cursor that circles (phx_world_set_link_anchors once per step) — the soft
 * counterpart of chain.c's pin drag.  Pins and links are solved in one pass on one schedule, which is built once.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/bridge.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o bridge
 *   ./bridge [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a joint that came apart, a rod that changed
 * its length, a schedule that was rebuilt).
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

#define PLANKS 8
#define PITCH 10.0f
#define DECK_Y 150.0f
#define HANGER 30.0f
#define ROPE 25.0f

/* the world point of `anchor` (body frame) on body b */
static void world_point(const phx_rigid_body* b, phx_vec2 anchor, float* x, float* y)
{
    *x = b->pos.x + b->xvector.x * anchor.x + b->yvector.x * anchor.y;
    *y = b->pos.y + b->xvector.y * anchor.x + b->yvector.y * anchor.y;
}

/* the distance between the two anchors of a pin or a link (body2 = -1: anchor2 is a world point) */
static float separation(const phx_rigid_body* bodies, int32_t body1, int32_t body2, phx_vec2 anchor1, phx_vec2 anchor2)
{
    float ax, ay, bx = anchor2.x, by = anchor2.y;
    world_point(&bodies[body1], anchor1, &ax, &ay);
    if (body2 >= 0) world_point(&bodies[body2], anchor2, &bx, &by);
    return hypotf(bx - ax, by - ay);
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const float half_span = PITCH * PLANKS / 2.0f;
    int32_t post[2], plank[PLANKS];
    for (int k = 0; k < 2; ++k) {
        post[k] = phx_world_add_body(world, (k ? 1.0f : -1.0f) * (half_span + 5.0f), DECK_Y, 0.0f, 5.0f, 5.0f);
        if (post[k] < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
        TRY(phx_world_set_body_static(world, post[k]));
    }
    for (int k = 0; k < PLANKS; ++k) {
        plank[k] = phx_world_add_body(world, -half_span + PITCH * ((float)k + 0.5f), DECK_Y, 0.0f, 4.0f, 1.0f);
        if (plank[k] < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    }
    const int32_t crate = phx_world_add_body(world, 0.0f, DECK_Y - 20.0f, 0.0f, 3.0f, 3.0f);
    const int32_t box = phx_world_add_body(world, 80.0f, DECK_Y, 0.0f, 3.0f, 3.0f);
    if (crate < 0 || box < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }

    /* the deck: post - plank - ... - plank - post */
    phx_pin pins[PLANKS + 1];
    const phx_vec2 near_end = { -PITCH / 2.0f, 0.0f }, far_end = { PITCH / 2.0f, 0.0f }, zero = { 0.0f, 0.0f };
    for (int k = 0; k <= PLANKS; ++k) {
        pins[k].impulse = zero;
        if (k < PLANKS) { pins[k].body1 = plank[k]; pins[k].anchor1 = near_end; }
        else { pins[k].body1 = plank[PLANKS - 1]; pins[k].anchor1 = far_end; }
        if (k == 0) { pins[k].body2 = post[0]; pins[k].anchor2.x = 5.0f; pins[k].anchor2.y = 0.0f; }
        else if (k == PLANKS) { pins[k].body2 = post[1]; pins[k].anchor2.x = -5.0f; pins[k].anchor2.y = 0.0f; }
        else { pins[k].body2 = plank[k - 1]; pins[k].anchor2 = far_end; }
    }
    TRY(phx_world_add_pins(world, pins, PLANKS + 1, NULL));

    /* the links: a rod per plank, the crate's rope, the box's spring.  The kind follows from the data: min == max is a rod, with
       hertz > 0 a spring; min < max are limits, and a rope is min = 0 */
    phx_link links[PLANKS + 2];
    for (int k = 0; k < PLANKS + 2; ++k) {
        links[k].body2 = -1; links[k].anchor1 = zero; links[k].hertz = 0.0f; links[k].damping_ratio = 0.0f; links[k].impulse = 0.0f; links[k].reserved = 0u;
    }
    for (int k = 0; k < PLANKS; ++k) {
        links[k].body1 = plank[k];
        links[k].anchor2.x = -half_span + PITCH * ((float)k + 0.5f); links[k].anchor2.y = DECK_Y + HANGER;
        links[k].min_length = links[k].max_length = HANGER;
    }
    const int rope = PLANKS, spring = PLANKS + 1;
    links[rope].body1 = crate; links[rope].anchor1.y = 3.0f;                                 /* from the crate's top ... */
    links[rope].body2 = plank[PLANKS / 2]; links[rope].anchor2.x = -PITCH / 2.0f; links[rope].anchor2.y = -1.0f;   /* ... to the underside of the deck's middle */
    links[rope].min_length = 0.0f; links[rope].max_length = ROPE;
    links[spring].body1 = box; links[spring].anchor2.x = 80.0f; links[spring].anchor2.y = DECK_Y;
    links[spring].min_length = links[spring].max_length = 5.0f; links[spring].hertz = 2.0f; links[spring].damping_ratio = 0.7f;
    int32_t first = -1;
    TRY(phx_world_add_links(world, links, PLANKS + 2, &first));
    TRY(phx_world_set_pin_iterations(world, 16));
    const int32_t spring_link = first + spring;

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    if (!bodies) return 1;
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    float worst_pin = 0.0f, worst_rod = 0.0f, cx = 80.0f, cy = DECK_Y;
    int slack = 0, taut = 0;
    for (int s = 0; s < steps; ++s) {
        const float t = (float)s * dt;
        cx = 80.0f + 10.0f * sinf(t);
        cy = DECK_Y + 15.0f - 10.0f * cosf(t);
        const float anchors[4] = { 0.0f, 0.0f, cx, cy };
        TRY(phx_world_set_link_anchors(world, &spring_link, anchors, 1));
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_bodies(world, bodies, nb));
        for (int k = 0; k <= PLANKS; ++k) {
            const float d = separation(bodies, pins[k].body1, pins[k].body2, pins[k].anchor1, pins[k].anchor2);
            if (d > worst_pin) worst_pin = d;
        }
        for (int k = 0; k < PLANKS; ++k) {
            const float e = fabsf(separation(bodies, links[k].body1, -1, links[k].anchor1, links[k].anchor2) - HANGER);
            if (e > worst_rod) worst_rod = e;
        }
        /* a limit engages the step after the length overshoots it: the rope is taut where it is at or past its length */
        if (separation(bodies, crate, links[rope].body2, links[rope].anchor1, links[rope].anchor2) < ROPE) slack = 1; else taut = 1;
    }
    phx_link got[PLANKS + 2];
    int32_t nl = 0, np = 0;
    TRY(phx_world_link_count(world, &nl));
    TRY(phx_world_pin_count(world, &np));
    if (nl != PLANKS + 2) { fprintf(stderr, "%d links\n", nl); return 1; }
    TRY(phx_world_get_links(world, got, nl));
    const float off = hypotf(bodies[box].pos.x - cx, bodies[box].pos.y - cy);
    int64_t builds = 0;
    TRY(phx_world_pin_schedule_builds(world, &builds));
    printf("bridge: %d pins and %d links after %d steps, largest pin separation %.4f, largest rod length error %.4f\n", np, nl, steps, worst_pin, worst_rod);
    printf("rope: slack %s, taut %s, impulse %.6f; the spring's box is %.3f from the cursor; the schedule was built %lld time(s)\n", slack ? "yes" : "no",
           taut ? "yes" : "no", got[rope].impulse, off, (long long)builds);
    free(bodies);
    phx_world_destroy(world);
    if (!(worst_pin < PITCH / 4.0f)) { fprintf(stderr, "a joint came apart\n"); return 1; }
    if (!(worst_rod < HANGER / 10.0f)) { fprintf(stderr, "a rod changed its length\n"); return 1; }
    if (builds != 1) { fprintf(stderr, "an edit rebuilt the schedule\n"); return 1; }
    return 0;
}
