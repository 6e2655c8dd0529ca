/*
 * chain.c — pins from plain C (include/phyx_amd.h PINS): a 12-link chain hung from a fixed point of the world swings down and comes to
 * rest on a stack of boxes, and one box of the stack is dragged by a world pin whose anchor follows a cursor (phx_world_set_pin_anchors
 * once per step) — the rigid counterpart of pick.c's acceleration drag.  The links share a negative collision group, so neighbours do
 * not collide with each other (pins do not stop that; collision filters do); they still collide with the stack.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/chain.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o chain
 *   ./chain [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a joint that came apart, a dragged box that
 * lost its cursor).
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

#define LINKS 12
#define SPACING 10.0f

/* the world point of `anchor` (body frame) on body b */
static void world_point(const phx_rigid_body* b, phx_vec2 anchor, float* x, float* y)
{
    *x = b->pos.x + b->xvector.x * anchor.x + b->yvector.x * anchor.y;
    *y = b->pos.y + b->xvector.y * anchor.x + b->yvector.y * anchor.y;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 600;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 10000.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    /* a stack of 3 x 4 boxes under the chain's free end, and one box beside it for the cursor */
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 4; ++r)
            if (phx_world_add_body(world, 60.0f + 12.0f * (float)c, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int32_t dragged = phx_world_add_body(world, -60.0f, 15.0f, 0.0f, 5.0f, 5.0f);
    /* the chain: links of 8 x 2 laid level with the fixed point (0, 120), to its right */
    const float top_x = 0.0f, top_y = 120.0f;
    int32_t link[LINKS];
    for (int k = 0; k < LINKS; ++k) {
        link[k] = phx_world_add_body(world, top_x + SPACING * ((float)k + 0.5f), top_y, 0.0f, 4.0f, 1.0f);
        if (link[k] < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    }
    phx_collision_filter no_self[LINKS];
    for (int k = 0; k < LINKS; ++k) { no_self[k].category = 1u; no_self[k].mask = 0xFFFFFFFFu; no_self[k].group = -1; }
    TRY(phx_world_set_collision_filters(world, link, no_self, LINKS, NULL));

    phx_pin pins[LINKS + 1];
    const phx_vec2 near_end = { -SPACING / 2.0f, 0.0f }, far_end = { SPACING / 2.0f, 0.0f }, zero = { 0.0f, 0.0f };
    for (int k = 0; k < LINKS; ++k) {
        pins[k].body1 = link[k]; pins[k].anchor1 = near_end; pins[k].impulse = zero;
        if (k == 0) { pins[k].body2 = -1; pins[k].anchor2.x = top_x; pins[k].anchor2.y = top_y; }
        else { pins[k].body2 = link[k - 1]; pins[k].anchor2 = far_end; }
    }
    /* the drag: the box's centre on the cursor */
    pins[LINKS].body1 = dragged; pins[LINKS].body2 = -1; pins[LINKS].anchor1 = zero; pins[LINKS].anchor2.x = -60.0f; pins[LINKS].anchor2.y = 15.0f;
    pins[LINKS].impulse = zero;
    int32_t first = -1;
    TRY(phx_world_add_pins(world, pins, LINKS + 1, &first));
    /* a long chain needs more than the default 8 sweeps: the bias is accumulated into the warm start, and a tension that the sweeps
       have not carried from one end to the other by the end of a step feeds an oscillation that grows (include/phyx_amd.h PINS) */
    TRY(phx_world_set_pin_iterations(world, 32));
    const int32_t drag_pin = first + LINKS;

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    float cx = -60.0f, cy = 15.0f;
    for (int s = 0; s < steps; ++s) {
        /* the cursor lifts the box and carries it along an ellipse, a quarter of a unit per step: the pin's bias closes a fifth of the gap
           per step, so the box trails the cursor by about five steps' travel */
        const float t = (float)s * dt;
        cx = -60.0f - 20.0f * sinf(0.5f * t);
        cy = 45.0f - 30.0f * cosf(0.5f * t);
        const float anchors[4] = { 0.0f, 0.0f, cx, cy };
        TRY(phx_world_set_pin_anchors(world, &drag_pin, anchors, 1));
        TRY(phx_world_update(world, dt, &cfg));
    }

    int32_t nb = 0, np = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    TRY(phx_world_pin_count(world, &np));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    phx_pin* got = (phx_pin*)malloc((size_t)np * sizeof *got);
    if (!bodies || !got) return 1;
    TRY(phx_world_get_bodies(world, bodies, nb));
    TRY(phx_world_get_pins(world, got, np));
    float worst = 0.0f, speed = 0.0f, lowest = top_y;
    for (int k = 0; k < LINKS; ++k) {                                        /* the chain's joints (the drag pin trails its cursor: below) */
        float ax, ay, bx = got[k].anchor2.x, by = got[k].anchor2.y;
        world_point(&bodies[got[k].body1], got[k].anchor1, &ax, &ay);
        if (got[k].body2 >= 0) world_point(&bodies[got[k].body2], got[k].anchor2, &bx, &by);
        const float d = hypotf(bx - ax, by - ay);
        if (d > worst) worst = d;
    }
    for (int k = 0; k < LINKS; ++k) {
        const phx_rigid_body* b = &bodies[link[k]];
        const float v = hypotf(b->velocity.x, b->velocity.y);
        if (v > speed) speed = v;
        if (b->pos.y < lowest) lowest = b->pos.y;
    }
    const float off = hypotf(bodies[dragged].pos.x - cx, bodies[dragged].pos.y - cy);
    int64_t builds = 0;
    TRY(phx_world_pin_schedule_builds(world, &builds));
    printf("chain: %d pins after %d steps, largest anchor separation %.4f, fastest link %.3f, lowest link at y %.2f\n", np, steps, worst, speed, lowest);
    printf("drag: box %d is %.4f from the cursor (%.2f, %.2f); the pin schedule was built %lld time(s)\n", dragged, off, cx, cy, (long long)builds);
    free(bodies); free(got);
    phx_world_destroy(world);
    if (!(worst < SPACING / 4.0f)) { fprintf(stderr, "a joint came apart\n"); return 1; }
    if (!(off < 3.0f)) { fprintf(stderr, "the dragged box lost its cursor\n"); return 1; }
    if (builds != 1) { fprintf(stderr, "anchor edits rebuilt the schedule\n"); return 1; }
    return 0;
}
