/*
 * rollback.c — rollback with device snapshots, through the C ABI: the demo loop of drag.c (ref: src/main.cpp:337-349) keeps a ring of
 * the last 8 frames' worlds in HBM (phx_world_save, one kernel per frame, nothing over PCIe).  Every 20th frame it goes back 6 frames
 * (phx_world_load), re-applies the inputs it recorded for those frames — the drag's accelerations — and simulates them again, as
 * rollback netcode does when a late input arrives.  The re-simulated frames must equal the first pass bit for bit: a checksum of
 * phx_world_get_poses after every frame says so.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/rollback.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -o rollback
 *   ./rollback [frames]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 2 a re-simulated frame differs, 1 any other failure.
 */
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

enum { RING = 8, BACK = 6, EVERY = 20, MAX_BODIES = 64 };

static const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };      /* ref: main.cpp:348 */
static const float dt = 1.0f / 60.0f;

/* FNV-1a over the poses of every body */
static int pose_checksum(phx_world* world, int bodies, uint64_t* out)
{
    static float poses[4 * MAX_BODIES];
    TRY(phx_world_get_poses(world, poses, bodies));
    const unsigned char* p = (const unsigned char*)poses;
    uint64_t h = 1469598103934665603ull;
    for (size_t k = 0; k < sizeof(float) * 4 * (size_t)bodies; ++k) { h ^= p[k]; h *= 1099511628211ull; }
    *out = h;
    return 0;
}

/* one frame: the recorded input, then World::Update */
static int frame(phx_world* world, int32_t dragged, const float accel[3])
{
    TRY(phx_world_add_accelerations(world, &dragged, accel, 1));
    TRY(phx_world_update(world, dt, &cfg));
    return 0;
}

int main(int argc, char** argv)
{
    const int frames = argc > 1 ? atoi(argv[1]) : 120;
    const float gravity = -200.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    if (frames < 1) { fprintf(stderr, "usage: rollback [frames >= 1]\n"); return 1; }

    /* the ground, the dragged box and a small stack for it to plough through */
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 10000.0f, 10.0f);
    const int dragged = phx_world_add_body(world, -120.0f, 60.0f, 0.0f, 12.0f, 12.0f);
    if (ground != 0 || dragged != 1) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int c = 0; c < 5; ++c)
        for (int r = 0; r < 6; ++r)
            if (phx_world_add_body(world, 12.0f * (float)c - 30.0f, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    int32_t bodies = 0;
    TRY(phx_world_counts(world, &bodies, NULL, NULL, NULL));
    if (bodies > MAX_BODIES) { fprintf(stderr, "too many bodies\n"); return 1; }

    phx_snapshot* ring[RING];
    for (int k = 0; k < RING; ++k) TRY(phx_snapshot_create(&ring[k], 0));
    float (*inputs)[3] = malloc(sizeof(float[3]) * (size_t)frames);      /* the recorded drag of every frame */
    uint64_t* sums = malloc(sizeof(uint64_t) * (size_t)frames);          /* the first pass's checksum after every frame */
    if (!inputs || !sums) { fprintf(stderr, "out of memory\n"); return 1; }

    int rollbacks = 0, resimulated = 0;
    const int32_t which[1] = { dragged };
    for (int f = 0; f < frames; ++f) {
        /* the world at the start of frame f goes into the ring: queued on the world's stream, no host wait */
        TRY(phx_world_save(world, ring[f % RING]));
        /* the input: drag body 1 to the right through the stack (ref: main.cpp:343-346) */
        phx_rigid_body b;
        TRY(phx_world_get_body_states(world, which, 1, &b));
        inputs[f][0] = (120.0f - b.velocity.x) * 5.0f;
        inputs[f][1] = -gravity + (0.0f - b.velocity.y) * 5.0f;
        inputs[f][2] = 0.0f;
        if (frame(world, dragged, inputs[f])) return 1;
        if (pose_checksum(world, bodies, &sums[f])) return 1;

        if (f % EVERY == EVERY - 1 && f >= BACK - 1) {
            /* a late input arrived: back to the start of frame f - 5, and the last 6 frames again from their recorded inputs */
            const int from = f - (BACK - 1);
            TRY(phx_world_load(world, ring[from % RING]));
            for (int g = from; g <= f; ++g) {
                uint64_t again = 0;
                if (frame(world, dragged, inputs[g])) return 1;
                if (pose_checksum(world, bodies, &again)) return 1;
                if (again != sums[g]) {
                    fprintf(stderr, "frame %d re-simulated from frame %d differs from the first pass (%016llx vs %016llx)\n", g, from,
                            (unsigned long long)again, (unsigned long long)sums[g]);
                    return 2;
                }
                ++resimulated;
            }
            ++rollbacks;
            printf("frame %3d: rolled back to frame %3d, re-simulated frame %3d equals the first pass (checksum %016llx)\n", f, from, f, (unsigned long long)sums[f]);
        }
    }
    int32_t sb = 0, sm = 0, scp = 0, sj = 0;
    TRY(phx_snapshot_counts(ring[(frames - 1) % RING], &sb, &sm, &scp, &sj));
    size_t blob = 0;
    TRY(phx_snapshot_blob_bytes(ring[(frames - 1) % RING], &blob));
    printf("last snapshot: %d bodies %d manifolds %d contact points %d joints, %zu bytes as a blob\n", sb, sm, scp, sj, blob);
    printf("rollback: %d rollbacks, %d re-simulated frames, all equal to the first pass\n", rollbacks, resimulated);
    for (int k = 0; k < RING; ++k) phx_snapshot_destroy(ring[k]);
    phx_world_destroy(world);
    free(inputs); free(sums);
    return 0;
}
