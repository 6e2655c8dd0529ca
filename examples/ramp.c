/*
 * ramp.c — convex polygon bodies from plain C (include/phyx_amd.h POLYGONS, PHX_SHAPE_POLYGON).
 *   the ramp:  a static triangular wedge whose face falls by 1 in 2 (steeper than the default friction holds), and below its foot a
 *              static trapezoid tray closed by a wall.
 *   on it:     three boxes that slide down the face, three marbles that roll down it and a hexagon that tumbles; all end in the tray.
 * add_polygons below is phyx_amd.World.add_polygons in C, three calls: phx_world_add_bodies with the frame box's half extents
 * (max |x|, max |y| of the vertices), phx_world_set_polygons to give the bodies their outlines, phx_world_set_inverse_masses.
 * The example prints where things end, how many manifolds on the ramp's face had two points while the bodies were on it, and a ray
 * cast down onto the slope with the normal it finds there.
 *
 *   gcc -std=c11 -O2 -Iinclude examples/ramp.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -lm -o ramp
 *   ./ramp [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (a body lost, a polygon that did not read
 * back, a ray that does not find the slope).
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

#define MOVERS 7

/* one polygon body at (px, py) turned by `angle`; inverse masses by the shoelace formulas on AddBody's scale (phyx_amd.polygon_inverse_masses) */
static int add_polygon(phx_world* world, float px, float py, float angle, const phx_polygon* p, int32_t* body)
{
    float hx = 0.f, hy = 0.f;
    double area = 0.0, second = 0.0;
    for (int k = 0; k < p->count; ++k) {
        const phx_vec2 a = p->v[k], b = p->v[(k + 1) % p->count];
        const double c = (double)a.x * b.y - (double)b.x * a.y;
        area += 0.5 * c;
        second += c * ((double)a.x * a.x + (double)a.y * a.y + (double)a.x * b.x + (double)a.y * b.y + (double)b.x * b.x + (double)b.y * b.y) / 12.0;
        hx = fabsf(a.x) > hx ? fabsf(a.x) : hx; hy = fabsf(a.y) > hy ? fabsf(a.y) : hy;
    }
    const double mass = 1e-5 * area / 4.0, inertia = 3.0 * mass * second / area;
    const float row[5] = { px, py, angle, hx, hy }, masses[2] = { 1.0f / (float)mass, 1.0f / (float)inertia };
    int st = phx_world_add_bodies(world, row, 1, body);                                      /* 1. a box of the frame's half extents */
    if (st == PHX_OK) st = phx_world_set_polygons(world, body, p, 1);                        /* 2. ... becomes the polygon */
    if (st == PHX_OK) st = phx_world_set_inverse_masses(world, body, masses, 1);             /* 3. ... with the polygon's mass */
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
    /* the wedge: its face runs from (-30, 22) down to (30, -8), y = 7 - x / 2; the tray's top is y = -10 from x = 30 to 110; a wall */
    const phx_polygon wedge = { 3, { { -30.f, -8.f }, { 30.f, -8.f }, { -30.f, 22.f } } };
    const phx_polygon tray = { 4, { { -38.f, -4.f }, { 38.f, -4.f }, { 40.f, 4.f }, { -40.f, 4.f } } };
    int32_t ramp = -1, floor_ = -1;
    TRY(add_polygon(world, 0.f, 0.f, 0.f, &wedge, &ramp));
    TRY(add_polygon(world, 70.f, -14.f, 0.f, &tray, &floor_));
    const int32_t wall = phx_world_add_body(world, 113.0f, 2.0f, 0.0f, 3.0f, 16.0f);
    if (wall < 0) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    const int32_t statics[3] = { ramp, floor_, wall };
    for (int k = 0; k < 3; ++k) TRY(phx_world_set_body_static(world, statics[k]));

    /* on the face at x: the surface point (x, 7 - x / 2) and the face's normal (1, 2) / sqrt(5) */
    const float slope = -atanf(0.5f), nx = 0.4472136f, ny = 0.8944272f;
    int32_t first = -1, movers[MOVERS];
    int made = 0;
    for (int k = 0; k < 3; ++k) {                                                           /* boxes {3, 2}, lying on the face */
        const float x = -20.f + 12.f * (float)k, lift = 2.0f - 0.05f;
        const float row[5] = { x + nx * lift, 7.f - 0.5f * x + ny * lift, slope, 3.0f, 2.0f };
        TRY(phx_world_add_bodies(world, row, 1, &first));
        movers[made++] = first;
    }
    for (int k = 0; k < 3; ++k) {                                                           /* marbles of radius 2.5 */
        const float x = -26.f + 12.f * (float)k, r = 2.5f, lift = r - 0.05f;
        const float row[5] = { x + nx * lift, 7.f - 0.5f * x + ny * lift, 0.f, r, r };
        TRY(phx_world_add_bodies(world, row, 1, &first));
        const phx_shape circle = { PHX_SHAPE_CIRCLE, r, r };
        const float mass = 1e-5f * 0.785398f * r * r, masses[2] = { 1.0f / mass, 1.0f / (mass * 1.5f * r * r) };
        TRY(phx_world_set_shapes(world, &first, &circle, 1));
        TRY(phx_world_set_inverse_masses(world, &first, masses, 1));
        movers[made++] = first;
    }
    {                                                                                       /* a hexagon of circumradius 4, a face on the slope */
        phx_polygon hexagon = { 6, { { 0 } } };
        for (int k = 0; k < 6; ++k) { hexagon.v[k].x = 4.0f * cosf(1.0471976f * (float)k); hexagon.v[k].y = 4.0f * sinf(1.0471976f * (float)k); }
        const float x = 16.f, lift = 4.0f * 0.8660254f - 0.05f;
        TRY(add_polygon(world, x + nx * lift, 7.f - 0.5f * x + ny * lift, slope, &hexagon, &first));
        movers[made++] = first;
    }

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    int on_face = 0;
    for (int s = 0; s < steps; ++s) {
        TRY(phx_world_update(world, dt, &cfg));
        if (s == 9) {                                                                       /* the bodies are still on the face: who lies on it with two points? */
            int32_t nm = 0;
            TRY(phx_world_counts(world, NULL, &nm, NULL, NULL));
            phx_manifold* manifolds = (phx_manifold*)malloc((size_t)(nm > 0 ? nm : 1) * sizeof *manifolds);
            if (!manifolds) return 1;
            TRY(phx_world_get_manifolds(world, manifolds, nm));
            for (int32_t k = 0; k < nm; ++k)
                on_face += (manifolds[k].body1 == ramp || manifolds[k].body2 == ramp) && manifolds[k].point_count == 2;
            free(manifolds);
        }
    }

    int32_t nb = 0;
    TRY(phx_world_counts(world, &nb, NULL, NULL, NULL));
    phx_rigid_body* bodies = (phx_rigid_body*)malloc((size_t)nb * sizeof *bodies);
    phx_shape* shapes = (phx_shape*)malloc((size_t)nb * sizeof *shapes);
    if (!bodies || !shapes) return 1;
    TRY(phx_world_get_bodies(world, bodies, nb));
    TRY(phx_world_get_shapes(world, shapes, nb));
    phx_polygon back[2];
    const int32_t ask[2] = { ramp, wall };
    TRY(phx_world_get_polygons(world, ask, back, 2));

    int polygons = 0, in_tray = 0, lost = 0;
    for (int32_t b = 0; b < nb; ++b) polygons += shapes[b].kind == PHX_SHAPE_POLYGON;
    for (int k = 0; k < MOVERS; ++k) {
        const phx_rigid_body* m = &bodies[movers[k]];
        if (!(m->pos.y > -12.0f && m->pos.y < 60.0f && m->pos.x > -40.0f && m->pos.x < 112.0f)) ++lost;      /* (a NaN counts as lost) */
        else if (m->pos.x > 30.0f && m->pos.y < 2.0f) ++in_tray;
    }
    /* straight down onto the top of the slope, where nothing is left: the face is at height 7 + 14 = 21 there */
    const float ray[5] = { -28.0f, 60.0f, 0.0f, -1.0f, 100.0f };
    phx_ray_hit hit;
    TRY(phx_world_raycast(world, ray, 1, 0, &hit));
    printf("ramp: %d polygons after %d steps; %d of %d bodies in the tray, %d lost\n", polygons, steps, in_tray, MOVERS, lost);
    printf("face: %d manifolds with two points on the ramp after 10 steps\n", on_face);
    printf("ray: down at x = -28 hits body %d at height %.4f, normal (%.4f, %.4f)\n", hit.body, hit.point.y, hit.normal.x, hit.normal.y);
    free(bodies); free(shapes);
    phx_world_destroy(world);
    if (polygons != 3 || back[0].count != 3 || back[1].count != 0) { fprintf(stderr, "%d polygons read back, 3 were made\n", polygons); return 1; }
    if (lost) { fprintf(stderr, "%d bodies left the scene\n", lost); return 1; }
    if (hit.body != ramp || fabsf(hit.point.y - 21.0f) > 0.01f || fabsf(hit.normal.x - nx) > 1e-4f || fabsf(hit.normal.y - ny) > 1e-4f) {
        fprintf(stderr, "the ray does not find the slope\n");
        return 1;
    }
    return 0;
}
