/*
 * rest.c — a pile that comes to rest, through the C ABI: boxes rain onto a static shelf with sleeping enabled
 * (phx_world_set_sleeping); the loop prints the asleep count each second until the whole pile rests.  Then a crate is dropped on it:
 * the component it hits wakes, everything else sleeps on, and the loop prints who woke (phx_world_get_sleep_states).
 *
 *   gcc -std=c11 -O2 -Iinclude examples/rest.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o rest
 *   ./rest [columns] [rows] [max seconds]
 *
 * The tolerances are the caller's units: here boxes of half-size 5 under gravity -200, whose piles creep at about 0.2 units/s and
 * 0.01 rad/s when they rest; 2.5 times that is calm, and half a second of calm is rest.
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure.
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

int main(int argc, char** argv)
{
    const int columns = argc > 1 ? atoi(argv[1]) : 6;
    const int rows = argc > 2 ? atoi(argv[2]) : 3;
    const int max_seconds = argc > 3 ? atoi(argv[3]) : 20;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (columns < 1 || columns > 1000 || rows < 1 || rows > 100 || max_seconds < 1) { fprintf(stderr, "usage: rest [columns in 1..1000] [rows in 1..100] [max seconds >= 1]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    /* the shelf (body 0, made static), and above it `rows` rows of boxes: the columns 30 apart, so that they settle as separate little
     * piles — separate components, which sleep and wake on their own */
    const int boxes = columns * rows, n = boxes + 1;
    float* spawn = (float*)malloc(sizeof(float) * 5 * (size_t)(n + 1));
    phx_sleep_state* before = (phx_sleep_state*)malloc(sizeof(phx_sleep_state) * (size_t)(n + 1));
    phx_sleep_state* after = (phx_sleep_state*)malloc(sizeof(phx_sleep_state) * (size_t)(n + 1));
    if (!spawn || !before || !after) { fprintf(stderr, "out of memory\n"); return 1; }
    spawn[0] = 0.0f; spawn[1] = 0.0f; spawn[2] = 0.0f; spawn[3] = 15.0f * (float)columns + 30.0f; spawn[4] = 10.0f;
    for (int c = 0; c < columns; ++c)
        for (int r = 0; r < rows; ++r) {
            float* q = spawn + 5 * (1 + c * rows + r);
            q[0] = 30.0f * ((float)c - 0.5f * (float)(columns - 1));
            q[1] = 16.0f + 11.0f * (float)r;                /* a unit above where it will rest: each box drops onto the one below */
            q[2] = 0.0f;
            q[3] = 5.0f; q[4] = 5.0f;
        }
    int32_t first = -1;
    TRY(phx_world_add_bodies(world, spawn, n, &first));
    const int32_t shelf[1] = { 0 };
    const float fixed[2] = { 0.0f, 0.0f };
    TRY(phx_world_set_inverse_masses(world, shelf, fixed, 1));

    const phx_sleep_params sleep = { 0.5f, 0.05f, 0.5f };
    TRY(phx_world_set_sleeping(world, &sleep));
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };

    int32_t asleep = 0;
    int64_t slept = 0, woken = 0;
    int second = 0;
    for (; second < max_seconds && asleep < boxes; ++second) {
        for (int s = 0; s < 60; ++s) TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_sleep_counts(world, &asleep, &slept, &woken));
        printf("second %2d: %d of %d boxes asleep\n", second + 1, asleep, boxes);
    }
    if (asleep < boxes) printf("rest: the pile still moves after %d seconds (%d of %d asleep)\n", max_seconds, asleep, boxes);
    else printf("rest: the pile rests after %d seconds\n", second);

    /* a crate onto the middle column */
    TRY(phx_world_get_sleep_states(world, before, n));
    const int target = columns / 2;
    const float crate[5] = { 30.0f * ((float)target - 0.5f * (float)(columns - 1)), 80.0f + 10.0f * (float)rows, 0.0f, 6.0f, 6.0f };
    TRY(phx_world_add_bodies(world, crate, 1, &first));
    int any = 0;
    for (int s = 0; s < 240 && !any; ++s) {
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_sleep_states(world, after, n + 1));
        for (int i = 0; i < n; ++i)
            if (before[i].asleep && !after[i].asleep) {
                if (!any) printf("step %d after the drop: the crate (body %d) woke", s + 1, first);
                printf(" %d", i);
                any = 1;
            }
    }
    if (any) printf("\n");
    else printf("the crate woke nobody within 240 steps\n");
    TRY(phx_world_sleep_counts(world, &asleep, &slept, &woken));
    printf("rest: %d asleep now, %lld put to sleep and %lld woken in total\n", asleep, (long long)slept, (long long)woken);
    free(spawn); free(before); free(after);
    phx_world_destroy(world);
    return 0;
}
