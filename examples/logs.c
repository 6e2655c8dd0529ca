/*
 * logs.c — capsule bodies from plain C (include/phyx_amd.h SHAPES, PHX_SHAPE_CAPSULE).
 *   the pile:  a dozen capsules dropped at mixed angles onto a static shelf between two posts; they come to rest as a pile of logs.
 *   the post:  one capsule stood on its end beside the pile with a small tilt; it topples and ends on its side.
 * add_capsules below is phyx_amd.World.add_capsules in C, three calls: phx_world_add_bodies with the frame box's half extents
 * (hx, hy), phx_world_set_shapes to make them capsules (radius hy, core segment hx - hy either way along x),
 * phx_world_set_inverse_masses with the capsule's mass and inertia on AddBody's scale.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/logs.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o logs
 *   ./logs [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a log left the shelf, a shape that did not
 * read back, the post still standing).
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

#define LOGS 12

/* rows = {px, py, angle, hx, hy} per capsule, hx > hy; *first = the index of the first new body */
static int add_capsules(phx_world* world, const float* rows, int32_t count, int32_t* first)
{
    int32_t* bodies = (int32_t*)malloc((size_t)count * sizeof(int32_t));
    phx_shape* shapes = (phx_shape*)malloc((size_t)count * sizeof(phx_shape));
    float* masses = (float*)malloc((size_t)count * 2 * sizeof(float));
    int st = bodies && shapes && masses ? PHX_OK : PHX_ERR_INVALID;
    for (int32_t k = 0; st == PHX_OK && k < count; ++k) {
        const float hx = rows[5 * k + 3], hy = rows[5 * k + 4];
        const float a = hx - hy, r = hy;                                                  /* include/phyx_amd.h SHAPES */
        shapes[k].kind = PHX_SHAPE_CAPSULE; shapes[k].hx = hx; shapes[k].hy = hy;
        const float mb = 1e-5f * a * r, mc = 1e-5f * 0.785398f * r * r;
        const float mass = mb + mc;
        const float inertia = mb * (a * a + r * r) + mc * (1.5f * r * r + 3.0f * a * a + 2.546479f * a * r);
        masses[2 * k] = 1.0f / mass; masses[2 * k + 1] = 1.0f / inertia;
    }
    if (st == PHX_OK) st = phx_world_add_bodies(world, rows, count, first);                  /* 1. boxes of half extents (hx, hy) */
    for (int32_t k = 0; st == PHX_OK && k < count; ++k) bodies[k] = *first + k;
    if (st == PHX_OK) st = phx_world_set_shapes(world, bodies, shapes, count);               /* 2. ... become capsules */
    if (st == PHX_OK) st = phx_world_set_inverse_masses(world, bodies, masses, count);       /* 3. ... with a capsule's mass */
    free(bodies); free(shapes); free(masses);
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
    /* the shelf and its two posts: static boxes */
    const int32_t shelf = phx_world_add_body(world, 40.0f, 0.0f, 0.0f, 110.0f, 3.0f);
    const int32_t left = phx_world_add_body(world, -33.0f, 43.0f, 0.0f, 3.0f, 40.0f);
    const int32_t right = phx_world_add_body(world, 33.0f, 43.0f, 0.0f, 3.0f, 40.0f);
    if (shelf < 0 || left < 0 || right < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int32_t statics[3] = { shelf, left, right };
    for (int k = 0; k < 3; ++k) TRY(phx_world_set_body_static(world, statics[k]));

    /* a dozen logs {10, 3} at mixed angles in six rows of two above the shelf; then the post, stood on its end beside the pen */
    float rows[(LOGS + 1) * 5];
    for (int k = 0; k < LOGS; ++k) {
        rows[5 * k] = (k % 2 ? 13.0f : -13.0f) + ((k / 2) % 2 ? 3.0f : -3.0f);
        rows[5 * k + 1] = 12.0f + 14.0f * (float)(k / 2);
        rows[5 * k + 2] = 0.35f * (float)((k * 5) % 7 - 3);
        rows[5 * k + 3] = 10.0f; rows[5 * k + 4] = 3.0f;
    }
    rows[5 * LOGS] = 90.0f; rows[5 * LOGS + 1] = 3.0f + 12.0f - 0.1f; rows[5 * LOGS + 2] = 1.5707963f + 0.1f;
    rows[5 * LOGS + 3] = 12.0f; rows[5 * LOGS + 4] = 2.5f;
    int32_t first = -1;
    TRY(add_capsules(world, rows, LOGS + 1, &first));
    const int32_t post = first + LOGS;

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    for (int s = 0; s < steps; ++s) TRY(phx_world_update(world, dt, &cfg));

    int32_t nb = 0, nm = 0;
    TRY(phx_world_counts(world, &nb, &nm, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    phx_shape* shapes = (phx_shape*)malloc((size_t)nb * sizeof *shapes);
    phx_manifold* manifolds = (phx_manifold*)malloc((size_t)(nm > 0 ? nm : 1) * sizeof *manifolds);
    if (!bodies || !shapes || !manifolds) return 1;
    TRY(phx_world_get_bodies(world, bodies, nb));
    TRY(phx_world_get_shapes(world, shapes, nb));
    TRY(phx_world_get_manifolds(world, manifolds, nm));

    int capsules = 0, resting = 0, lost = 0;
    for (int32_t b = 0; b < nb; ++b) capsules += shapes[b].kind == PHX_SHAPE_CAPSULE;
    for (int32_t b = first; b < first + LOGS; ++b) {
        const phx_rigid_body* m = &bodies[b];
        const float speed = sqrtf(m->velocity.x * m->velocity.x + m->velocity.y * m->velocity.y);
        if (!(m->pos.y > 3.0f && m->pos.y < 200.0f && fabsf(m->pos.x) < 30.0f)) ++lost;      /* (a NaN counts as lost) */
        if (speed < 1.0f && fabsf(m->angular_velocity) < 0.5f) ++resting;
    }
    /* the manifolds of the pile by their point counts: a log resting on a face or along another log has two points */
    int by_count[3] = { 0, 0, 0 };
    for (int32_t k = 0; k < nm; ++k) {
        const phx_manifold* m = &manifolds[k];
        if (m->body1 == post || m->body2 == post) continue;
        if (m->point_count >= 0 && m->point_count <= 2) ++by_count[m->point_count];
    }
    const float lean = fabsf(bodies[post].xvector.y);      /* |sin| of the post's angle: 1 standing, 0 on its side */
    printf("logs: %d capsules after %d steps; %d of %d logs at rest, %d lost\n", capsules, steps, resting, LOGS, lost);
    printf("pile: %d manifolds with two points, %d with one, %d with none\n", by_count[2], by_count[1], by_count[0]);
    printf("post: |sin(angle)| %.4f, its centre at height %.4f\n", lean, bodies[post].pos.y);
    free(bodies); free(shapes); free(manifolds);
    phx_world_destroy(world);
    if (capsules != LOGS + 1) { fprintf(stderr, "%d capsules read back, %d were made\n", capsules, LOGS + 1); return 1; }
    if (lost) { fprintf(stderr, "%d logs left the shelf\n", lost); return 1; }
    if (!(lean < 0.1f)) { fprintf(stderr, "the post is still standing\n"); return 1; }
    return 0;
}
