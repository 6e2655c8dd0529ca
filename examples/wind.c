/*
 * wind.c — force fields through the C ABI (phx_world_set_fields, phx_world_pulse_fields): columns of boxes drop through a box-shaped
 * wind zone onto a shelf and land displaced downwind; a drag pool above the shelf slows what falls into it; at a fixed frame a radial
 * pulse — a blast — scatters the pile.  The fields are computed on the device from the bodies' own state: the loop below reads
 * bodies back only to print.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/wind.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o wind
 *   ./wind [columns] [rows] [frames]
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

static float speed(const phx_rigid_body* b) { return sqrtf(b->velocity.x * b->velocity.x + b->velocity.y * b->velocity.y); }

int main(int argc, char** argv)
{
    const int columns = argc > 1 ? atoi(argv[1]) : 8;
    const int rows = argc > 2 ? atoi(argv[2]) : 6;
    const int frames = argc > 3 ? atoi(argv[3]) : 480;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (columns < 1 || columns > 1000 || rows < 1 || rows > 100 || frames < 150) { fprintf(stderr, "usage: wind [columns in 1..1000] [rows in 1..100] [frames >= 150]\n"); return 1; }
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    /* the shelf (body 0, made static) and above it the columns, 30 apart, each box 12 above the one below */
    const int boxes = columns * rows, n = boxes + 1;
    const float width = 30.0f * (float)columns;
    float* spawn = (float*)malloc(sizeof(float) * 5 * (size_t)n);
    phx_rigid_body* before = (phx_rigid_body*)malloc(sizeof(phx_rigid_body) * (size_t)n);
    phx_rigid_body* now = (phx_rigid_body*)malloc(sizeof(phx_rigid_body) * (size_t)n);
    float* speed_in = (float*)calloc((size_t)n, sizeof(float));
    int* frame_in = (int*)calloc((size_t)n, sizeof(int));
    if (!spawn || !before || !now || !speed_in || !frame_in) { fprintf(stderr, "out of memory\n"); return 1; }
    spawn[0] = 0.0f; spawn[1] = 0.0f; spawn[2] = 0.0f; spawn[3] = width + 300.0f; spawn[4] = 10.0f;
    for (int c = 0; c < columns; ++c)
        for (int r = 0; r < rows; ++r) {
            float* q = spawn + 5 * (1 + c * rows + r);
            q[0] = 30.0f * ((float)c - 0.5f * (float)(columns - 1));
            q[1] = 220.0f + 12.0f * (float)r;
            q[2] = 0.0f;
            q[3] = 5.0f; q[4] = 5.0f;
        }
    int32_t first = -1;
    TRY(phx_world_add_bodies(world, spawn, n, &first));
    const int32_t shelf[1] = { 0 };
    const float fixed[2] = { 0.0f, 0.0f };
    TRY(phx_world_set_inverse_masses(world, shelf, fixed, 1));

    /* a wind to the right between y = 90 and y = 200, and a pool of drag from the shelf's top up to y = 70 */
    const float far = width + 300.0f;
    const phx_field fields[2] = {
        { PHX_FIELD_UNIFORM, PHX_REGION_BOX, 0xFFFFFFFFu, 0u, { -far, 90.0f, far, 200.0f }, { 250.0f, 0.0f, 0.0f, 0.0f } },
        { PHX_FIELD_DRAG, PHX_REGION_BOX, 0xFFFFFFFFu, 0u, { -far, 10.0f, far, 70.0f }, { 0.0f, 0.0f, 6.0f, 2.0f } },
    };
    TRY(phx_field_check(fields, 2));
    TRY(phx_world_set_fields(world, fields, 2));
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };

    /* every box's speed when it enters the pool and 8 frames later */
    const int blast_frame = frames - 60, lag = 8;
    double in_sum = 0.0, out_sum = 0.0;
    int measured = 0;
    for (int frame = 0; frame < blast_frame; ++frame) {
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_bodies(world, now, n));
        for (int i = 1; i < n; ++i) {
            if (!frame_in[i] && now[i].pos.y <= 70.0f) { frame_in[i] = frame + 1; speed_in[i] = speed(&now[i]); }
            else if (frame_in[i] && frame + 1 == frame_in[i] + lag) { in_sum += speed_in[i]; out_sum += speed(&now[i]); ++measured; }
        }
    }
    double shift = 0.0;
    for (int i = 1; i < n; ++i) shift += now[i].pos.x - spawn[5 * i];
    printf("wind: the boxes landed %.2f downwind of where they were dropped, on average\n", shift / boxes);
    if (measured) printf("pool: %d boxes entered at %.2f and were at %.2f %d frames later, on average\n", measured, in_sum / measured, out_sum / measured, lag);
    else printf("pool: no box reached the pool\n");

    /* the blast: a radial pulse under the middle of the pile, fading to nothing at 150 */
    double cx = 0.0;
    for (int i = 1; i < n; ++i) cx += now[i].pos.x;
    const phx_field blast[1] = { { PHX_FIELD_RADIAL, PHX_REGION_ALL, 0xFFFFFFFFu, 0u, { 0.0f, 0.0f, 0.0f, 0.0f }, { (float)(cx / boxes), 10.0f, 400.0f, 150.0f } } };
    TRY(phx_world_get_bodies(world, before, n));
    TRY(phx_world_pulse_fields(world, blast, 1));
    TRY(phx_world_get_bodies(world, now, n));
    int moved = 0;
    for (int i = 0; i < n; ++i) moved += fabsf(now[i].velocity.x - before[i].velocity.x) + fabsf(now[i].velocity.y - before[i].velocity.y) > 1.0f;
    printf("blast at frame %d: %d of %d boxes moved\n", blast_frame, moved, boxes);
    for (int frame = blast_frame; frame < frames; ++frame) TRY(phx_world_update(world, dt, &cfg));
    int64_t passes = 0;
    TRY(phx_world_field_passes(world, &passes));
    printf("wind: %d frames, %lld field passes\n", frames, (long long)passes);
    free(spawn); free(before); free(now); free(speed_in); free(frame_in);
    phx_world_destroy(world);
    return 0;
}
