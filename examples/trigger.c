/*
 * trigger.c — a sensor body in a demo loop: a static trigger zone hangs above the ground and boxes fall through it onto the ground.
 * The zone has PHX_BODY_SENSOR: its pairs have manifolds and contact points, so phx_world_contact_events reports a begin when a box
 * enters it and an end when the box has left it, but they get no joints, so the zone pushes nothing.  The same boxes are dropped a
 * second time in a world without the zone: they end at exactly the same heights.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/trigger.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o trigger
 *   ./trigger [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or the zone did not behave as described).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phyx_amd.h"

#define TRY(call)                                                                      \
    do {                                                                               \
        int st_ = (call);                                                              \
        if (st_ != PHX_OK) {                                                           \
            fprintf(stderr, "%s -> %d: %s\n", #call, st_, phx_last_error());           \
            return st_ == PHX_ERR_NO_DEVICE ? 3 : 1;                                   \
        }                                                                              \
    } while (0)

#define BOXES 3
#define MAX_BODIES (2 + BOXES)
#define MAX_EVENTS 64

/* the ground, the boxes (bodies 1 .. BOXES) and, if asked for, the zone as the last body; steps; the boxes' final poses into `poses`.
 * With the zone: every begin and end event of a (box, zone) pair is printed and counted per box. */
static int run(int with_zone, int steps, float* poses, int began[BOXES], int ended[BOXES])
{
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 1000.0f, 10.0f);
    if (ground != 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int b = 0; b < BOXES; ++b)
        if (phx_world_add_body(world, 30.0f * (float)b - 30.0f, 120.0f + 30.0f * (float)b, 0.0f, 5.0f, 5.0f) != 1 + b) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    int32_t zone = -1;
    if (with_zone) {
        zone = phx_world_add_body(world, 0.0f, 60.0f, 0.0f, 50.0f, 10.0f);
        if (zone != 1 + BOXES) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
        TRY(phx_world_set_body_static(world, zone));
        const uint32_t sensor = PHX_BODY_SENSOR;
        TRY(phx_world_set_body_flags(world, &zone, &sensor, 1));
    }
    for (int s = 0; s < steps; ++s) {
        TRY(phx_world_update(world, dt, &cfg));
        if (!with_zone) continue;
        int32_t begin[2 * MAX_EVENTS], end[2 * MAX_EVENTS];
        int64_t nbegin = 0, nend = 0;
        TRY(phx_world_contact_events(world, begin, MAX_EVENTS, &nbegin, end, MAX_EVENTS, &nend));
        for (int e = 0; e < (int)(nbegin + nend); ++e) {
            const int32_t* pair = e < (int)nbegin ? begin + 2 * e : end + 2 * (e - (int)nbegin);
            if (pair[0] != zone && pair[1] != zone) continue;
            const int box = pair[0] == zone ? pair[1] : pair[0];
            if (box < 1 || box > BOXES) continue;
            if (e < (int)nbegin) { ++began[box - 1]; printf("step %3d: box %d enters the zone\n", s, box); }
            else { ended[box - 1] += began[box - 1] > 0; printf("step %3d: box %d has left the zone\n", s, box); }
        }
    }
    TRY(phx_world_synchronize(world));
    if (with_zone) {
        /* the zone's contacts carry no joint: nothing was ever pushed */
        int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
        TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
        printf("with the zone: %d bodies, %d manifolds, %d joints\n", nb, nm, nj);
    }
    static float all[4 * MAX_BODIES];
    TRY(phx_world_get_poses(world, all, MAX_BODIES));
    memcpy(poses, all + 4, 4 * BOXES * sizeof(float));
    phx_world_destroy(world);
    return 0;
}

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 240;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    if (steps < 120) { fprintf(stderr, "usage: trigger [steps >= 120]\n"); return 1; }
    float with[4 * BOXES], without[4 * BOXES];
    int began[BOXES] = {0}, ended[BOXES] = {0}, unused[BOXES] = {0};
    int st = run(1, steps, with, began, ended);
    if (st) return st;
    st = run(0, steps, without, unused, unused);
    if (st) return st;
    int ok = 1;
    for (int b = 0; b < BOXES; ++b) {
        if (began[b] != 1 || ended[b] != 1) { fprintf(stderr, "box %d: %d begin and %d end events for the zone (1 and 1 expected)\n", 1 + b, began[b], ended[b]); ok = 0; }
        if (!(with[4 * b + 1] < 20.0f)) { fprintf(stderr, "box %d did not fall through the zone onto the ground (y %.3f)\n", 1 + b, with[4 * b + 1]); ok = 0; }
    }
    const int same = memcmp(with, without, sizeof with) == 0;
    printf("final heights %.4f %.4f %.4f; without the zone %.4f %.4f %.4f: %s\n", with[1], with[5], with[9], without[1], without[5], without[9],
           same ? "the same poses, bit for bit" : "DIFFERENT");
    if (!same) { fprintf(stderr, "the zone changed where the boxes ended\n"); ok = 0; }
    return ok ? 0 : 1;
}
