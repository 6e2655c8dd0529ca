/*
 * materials.c — per-body friction and restitution in a demo loop.  On the ground (default material {0.3, 0}) lie an ice shelf
 * (friction 0) with a box on it (friction 0 too), and a rubber box (restitution 0.8) is dropped next to it.  Once the box has settled on
 * the shelf it is given vx = 50: on ice nothing slows it down.  The rubber box hits the ground and rises again at most of its impact
 * speed (a contact uses the larger restitution of its two bodies).
 *
 *   gcc -std=c11 -O2 -Iinclude examples/materials.c -Lphyx_amd -lphyx_amd -Wl,-rpath,$PWD/phyx_amd -o materials
 *   ./materials [steps]
 *
 * Exit status: 0 ok, 3 no usable device (there is no CPU fallback), 1 any other failure (or the boxes did not behave as described).
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

int main(int argc, char** argv)
{
    const int steps = argc > 1 ? atoi(argv[1]) : 120;
    const float gravity = -200.0f, dt = 1.0f / 60.0f;
    if (phx_abi_version() != PHX_ABI_VERSION) { fprintf(stderr, "header / library ABI mismatch\n"); return 1; }
    if (steps < 90) { fprintf(stderr, "usage: materials [steps >= 90]\n"); return 1; }

    phx_world* world = NULL;
    TRY(phx_world_create(&world, 0));
    TRY(phx_world_set_gravity(world, gravity));
    const int ground = phx_world_add_body(world, 0.0f, 0.0f, 0.0f, 1000.0f, 10.0f);
    const int shelf = phx_world_add_body(world, -500.0f, 15.0f, 0.0f, 400.0f, 5.0f);
    const int slider = phx_world_add_body(world, -850.0f, 24.9f, 0.0f, 5.0f, 5.0f);
    const int rubber = phx_world_add_body(world, 300.0f, 200.0f, 0.0f, 5.0f, 5.0f);
    if (ground != 0 || shelf != 1 || slider != 2 || rubber != 3) { fprintf(stderr, "add_body: %s\n", phx_last_error()); return 1; }
    TRY(phx_world_set_body_static(world, ground));
    TRY(phx_world_set_body_static(world, shelf));

    /* before the first step: the materials go up with the bodies */
    const int32_t which[3] = { shelf, slider, rubber };
    const phx_material mats[3] = { { 0.0f, 0.0f }, { 0.0f, 0.0f }, { 0.3f, 0.8f } };
    TRY(phx_world_set_materials(world, which, mats, 3));

    const phx_config cfg = { PHX_SOLVE_AVX2, PHX_ISLAND_MULTIPLE_SLOPPY, 15, 15 };
    const int kick = 20;
    const int32_t both[2] = { slider, rubber };
    phx_rigid_body b[2];
    float v0 = 0.0f, vslide = 0.0f, impact = 0.0f, rise = 0.0f, prev_vy = 0.0f;
    for (int s = 0; s < steps; ++s) {
        if (s == kick) {
            const float vel[3] = { 50.0f, 0.0f, 0.0f };
            TRY(phx_world_set_velocities(world, &slider, vel, 1));
        }
        TRY(phx_world_update(world, dt, &cfg));
        TRY(phx_world_get_body_states(world, both, 2, b));
        if (s == kick) v0 = b[0].velocity.x;
        if (s == kick + 60) vslide = b[0].velocity.x;
        const float vy = b[1].velocity.y;
        if (vy < -impact && rise == 0.0f) impact = -vy;              /* falling: the fastest downward speed before the first rebound */
        if (prev_vy < 0.0f && vy > 0.0f && rise == 0.0f) {
            rise = vy;
            printf("step %3d: the rubber box hits the ground at %.1f and leaves it at %.1f\n", s, impact, rise);
        }
        prev_vy = vy;
    }
    printf("the box on the ice shelf: vx %.4f after the kick, %.4f sixty steps later\n", v0, vslide);
    phx_world_destroy(world);
    if (!(v0 > 49.9f && vslide > v0 - 1e-3f && vslide < v0 + 1e-3f)) { fprintf(stderr, "the box did not slide freely on the ice\n"); return 1; }
    if (!(impact > 100.0f && rise > 0.5f * impact)) { fprintf(stderr, "the rubber box did not bounce\n"); return 1; }
    printf("slide and bounce as described\n");
    return 0;
}
