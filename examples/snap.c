/*
 * snap.c — breakable joints from plain C (include/phyx_amd.h BREAKS): the deck of bridge.c, 8 planks pinned end to end between two
 * static posts with a rod hanger from every plank to a fixed point above it.  The hangers get a break limit of 8 times the largest
 * load one of them carries while the bridge hangs by itself; then crates drop on the middle of the deck, one after another, until
 * hangers snap.  The test runs on the device behind the pin pass; what comes down per step is a 4-byte count, and the events of the
 * steps that have some.  The program prints every event and the height of the deck's middle as it gives way.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/snap.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o snap
 *   ./snap [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (no hanger snapped, the deck did not drop).
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
#define CRATES 8
#define PITCH 10.0f
#define DECK_Y 150.0f
#define HANGER 30.0f
#define SETTLE 90

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

    /* the deck: post - plank - ... - plank - post; unbreakable, as every new unit is */
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

    /* a rod hanger per plank */
    phx_link links[PLANKS];
    for (int k = 0; k < PLANKS; ++k) {
        links[k].body1 = plank[k]; links[k].body2 = -1; links[k].anchor1 = zero;
        links[k].anchor2.x = -half_span + PITCH * ((float)k + 0.5f); links[k].anchor2.y = DECK_Y + HANGER;
        links[k].min_length = links[k].max_length = HANGER;
        links[k].hertz = 0.0f; links[k].damping_ratio = 0.0f; links[k].impulse = 0.0f; links[k].reserved = 0u;
    }
    TRY(phx_world_add_links(world, links, PLANKS, NULL));
    TRY(phx_world_set_pin_iterations(world, 16));

    /* the bridge hangs by itself for a while; the largest impulse a hanger transmits in a step then, over dt, is its static load */
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    for (int s = 0; s < SETTLE; ++s) TRY(phx_world_update(world, dt, &cfg));
    TRY(phx_world_get_links(world, links, PLANKS));
    float load = 0.0f;
    for (int k = 0; k < PLANKS; ++k) load = fmaxf(load, fabsf(links[k].impulse) / dt);
    if (!(load > 0.0f)) { fprintf(stderr, "the hangers carry nothing\n"); return 1; }
    int32_t which[PLANKS];
    float limits[PLANKS];
    for (int k = 0; k < PLANKS; ++k) { which[k] = k; limits[k] = 8.0f * load; }
    TRY(phx_world_set_break_limits(world, PHX_UNIT_LINK, which, limits, PLANKS));
    printf("snap: %d hangers, the most loaded carries %.5f; each breaks above %.5f\n", PLANKS, load, limits[0]);

    /* the crates, stacked in the air above the middle of the deck: they land one after another */
    const int middle = PLANKS / 2;
    for (int k = 0; k < CRATES; ++k)
        if (phx_world_add_body(world, -half_span + PITCH * ((float)middle + 0.5f), DECK_Y + 12.0f + 14.0f * (float)k, 0.0f, 3.0f, 3.0f) < 0) {
            fprintf(stderr, "add_body: %s\n", phx_last_error());
            return 1;
        }

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    if (!bodies) return 1;
    int snapped = 0;
    float lowest = DECK_Y;
    for (int s = 0; s < steps; ++s) {
        TRY(phx_world_update(world, dt, &cfg));
        /* once per step: every event then has step 0, and its index is the hanger's index before this step's removals */
        phx_break_event events[2 * PLANKS + 1];
        int64_t total = 0;
        TRY(phx_world_break_events(world, events, 2 * PLANKS + 1, &total));
        for (int64_t e = 0; e < total; ++e) {
            printf("step %3d: hanger %d of plank %d snapped: it transmitted %.5f, its limit allows %.5f\n", s, events[e].index, events[e].body1 - plank[0],
                   events[e].reaction / dt, events[e].threshold / dt);
            ++snapped;
        }
        if (total || s % 60 == 59) {
            TRY(phx_world_get_body_states(world, &plank[middle], 1, bodies));
            lowest = fminf(lowest, bodies[0].pos.y);
            printf("step %3d: the deck's middle is at %.2f\n", s, bodies[0].pos.y);
        }
    }
    int32_t nl = 0;
    int64_t builds = 0;
    TRY(phx_world_link_count(world, &nl));
    TRY(phx_world_pin_schedule_builds(world, &builds));
    printf("snap: %d of %d hangers snapped, %d hold; the deck's middle fell from %.2f to %.2f; the schedule was built %lld time(s)\n", snapped, PLANKS, nl, DECK_Y,
           lowest, (long long)builds);
    free(bodies);
    phx_world_destroy(world);
    if (!snapped || nl != PLANKS - snapped) { fprintf(stderr, "no hanger snapped\n"); return 1; }
    if (!(lowest < DECK_Y - 1.0f)) { fprintf(stderr, "the deck did not drop\n"); return 1; }
    return 0;
}
