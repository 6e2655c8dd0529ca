/*
 * contacts.c — the reference's demo loop with contact reports (ref: src/main.cpp:337-349 drags body 1; main.cpp:393-413 draws every
 * contact point at pos + delta with V held and marks the new ones).  Body 1 is dragged onto a stack as drag.c drags it.  After every
 * step the loop asks the world, on the device:
 *   - phx_world_contact_events: the pairs that started / stopped touching since the last call; those with body 1 are printed;
 *   - phx_world_query_contacts: body 1's contacts with their impulses (the ground left out with PHX_QUERY_SKIP_STATIC on odd steps);
 *   - phx_world_get_contact_markers_device: the demo's V view, into a device buffer a renderer would draw from.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/contacts.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o contacts
 *   ./contacts [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or body 1 never touched anything).
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

/* the drag target after `step` steps at `speed` units per step along the polyline px / py (n points) */
static void target_at(int step, float speed, const float* px, const float* py, int n, float* tx, float* ty)
{
    float left = speed * (float)step;
    for (int k = 0; k + 1 < n; ++k) {
        const float dx = px[k + 1] - px[k], dy = py[k + 1] - py[k];
        const float d = dx < 0 ? -dx : dx;
        const float e = dy < 0 ? -dy : dy;
        const float len = d > e ? d : e;                                     /* (axis-aligned legs) */
        if (left <= len) { *tx = px[k] + dx * (left / len); *ty = py[k] + dy * (left / len); return; }
        left -= len;
    }
    *tx = px[n - 1]; *ty = py[n - 1];
}

#define MAX_EVENTS 4096
#define MAX_CONTACTS 256

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 240;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }

    /* ref: main.cpp:88-95: the ground and the 30 x 30 box that the mouse drags; then a small stack */
    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 10000.0f, 10.0f);
    const int dragged = phx_world_add_body(world, -300.0f, 300.0f, 0.0f, 30.0f, 30.0f);
    if (ground != 0 || dragged != 1) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    for (int c = 0; c < 6; ++c)
        for (int r = 0; r < 8; ++r)
            if (phx_world_add_body(world, 12.0f * (float)c - 30.0f, 15.0f + 10.0f * (float)r, 0.0f, 5.0f, 5.0f) < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }

    /* down onto the ground, then along it into the stack */
    const float px[] = {-300.0f, -300.0f, 100.0f}, py[] = {300.0f, 40.0f, 40.0f};
    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };      /* ref: main.cpp:348 */
    const int32_t which[1] = { dragged };
    static int32_t begin[2 * MAX_EVENTS], end[2 * MAX_EVENTS];
    static phx_contact found[MAX_CONTACTS];
    void* d_markers = NULL;
    int32_t marker_cap = 0;
    int touched = 0;
    long long begins = 0, ends = 0;
    for (int s = 0; s < steps; ++s) {
        phx_rigid_body b;
        TRY(phx_world_get_body_states(world, which, 1, &b));                 /* RigidBody* draggedBody = &world.bodies[1] */
        float tx = 0.0f, ty = 0.0f;
        target_at(s, 6.0f, px, py, 3, &tx, &ty);
        const float dst_x = (tx - b.pos.x) * 5e1f, dst_y = (ty - b.pos.y) * 5e1f;
        float accel[3] = { 0.0f, 0.0f, 0.0f };
        accel[1] -= gravity;                                                 /* draggedBody->acceleration.y -= gravity */
        accel[0] += (dst_x - b.velocity.x) * 5.0f;                           /* draggedBody->acceleration += (dstVelocity - velocity) * 5 */
        accel[1] += (dst_y - b.velocity.y) * 5.0f;
        TRY(phx_world_add_accelerations(world, which, accel, 1));
        TRY(phx_world_update(world, dt, &cfg));

        /* who started / stopped touching whom since the last step */
        int64_t nbegin = 0, nend = 0;
        TRY(phx_world_contact_events(world, begin, MAX_EVENTS, &nbegin, end, MAX_EVENTS, &nend));
        begins += nbegin; ends += nend;
        for (int64_t k = 0; k < nbegin; ++k)
            if (begin[2 * k] == dragged || begin[2 * k + 1] == dragged) printf("step %3d: begin %d - %d\n", s, begin[2 * k], begin[2 * k + 1]);
        for (int64_t k = 0; k < nend; ++k)
            if (end[2 * k] == dragged || end[2 * k + 1] == dragged) printf("step %3d: end   %d - %d\n", s, end[2 * k], end[2 * k + 1]);

        /* body 1's contacts, every 30 steps */
        int32_t offsets[2];
        int64_t total = 0;
        const int32_t flags = (s & 1) ? PHX_QUERY_SKIP_STATIC : 0;
        TRY(phx_world_query_contacts(world, which, 1, flags, offsets, found, MAX_CONTACTS, &total));
        touched += total > 0;
        if (s % 30 == 29)
            for (int64_t k = 0; k < total; ++k)
                printf("step %3d: body 1 touches %d (manifold %d slot %d%s) at (%.2f, %.2f) normal (%.3f, %.3f) impulse %.3f / %.3f\n", s,
                       found[k].other, found[k].manifold, found[k].slot, (found[k].flags & PHX_CONTACT_NEW) ? ", new" : "", found[k].point.x,
                       found[k].point.y, found[k].normal.x, found[k].normal.y, found[k].normal_impulse, found[k].friction_impulse);

        /* the V view: two markers per manifold into device memory, grown as the manifolds grow */
        int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
        TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
        if (2 * nm > marker_cap) {
            if (d_markers) TRY(phx_device_free(0, d_markers));
            marker_cap = 4 * nm + 64;
            TRY(phx_device_malloc(0, (size_t)marker_cap * sizeof(phx_contact_marker), &d_markers));
        }
        TRY(phx_world_get_contact_markers_device(world, d_markers, marker_cap));
    }
    TRY(phx_world_synchronize(world));
    int32_t nb = 0, nm = 0, ncp = 0, nj = 0;
    TRY(phx_world_counts(world, &nb, &nm, &ncp, &nj));
    printf("world: %d bodies %d manifolds; %lld begin and %lld end events over %d steps; body 1 touched something in %d steps\n", nb, nm,
           begins, ends, steps, touched);
    if (d_markers) TRY(phx_device_free(0, d_markers));
    phx_world_destroy(world);
    if (!touched) { fprintf(stderr, "body 1 never touched anything\n"); return 1; }
    return 0;
}
