/*
 * phyx_amd.h — C ABI of the MI355X-native contact solver + sweep-and-prune broadphase.
 *
 * The reference (zeux/phyx) has no plugin/FFI layer; its de-facto boundary is what World::Update
 * calls (ref: src/World.cpp:19-37): Collider::UpdateBroadphase / UpdatePairs (src/Collider.h:28-29),
 * Solver::SolveJoints (src/Solver.h:54) and the Configuration struct (src/Configuration.h:3-23),
 * all operating on the public POD arrays RigidBody (src/RigidBody.h:12-57, 128 B), ContactPoint
 * (src/Manifold.h:12-43, 32 B), Manifold (src/Manifold.h:45-67, 16 B) and ContactJoint
 * (src/Joints.h:6-23, 20 B).  Every entry point below names the reference interface it replaces
 * and takes those exact layouts, so buffers can cross the boundary unchanged.
 *
 * Conventions: plain pointers and sizes only; every function returns PHX_OK (0) or a negative
 * phx_status (the reference's void/assert convention is the one deliberate deviation);
 * phx_last_error() gives the message of the last failure on the calling thread.  A handle is not
 * re-entrant (like the reference's member scratch, ref: src/Solver.h:108-128): one thread per
 * handle at a time.  Pointers are borrowed for the duration of the call only.
 *
 * There is no CPU fallback: every compute entry point fails with PHX_ERR_NO_DEVICE when no
 * gfx950 device is usable.
 */
#ifndef PHYX_AMD_H
#define PHYX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_ABI_VERSION 2

typedef enum {
    PHX_OK = 0,
    PHX_ERR_INVALID = -1,     /* bad argument / size / enum value                         */
    PHX_ERR_NO_DEVICE = -2,   /* no usable HIP device                                      */
    PHX_ERR_HIP = -3,         /* a HIP runtime call failed (see phx_last_error)            */
    PHX_ERR_CAPACITY = -4,    /* caller-provided output buffer too small                   */
    PHX_ERR_STATE = -5        /* call order violated (e.g. query before first solve)       */
} phx_status;

/* ref: src/Configuration.h:5-18 — same numeric values */
enum { PHX_SOLVE_SCALAR = 0, PHX_SOLVE_SSE2 = 1, PHX_SOLVE_AVX2 = 2 };
enum { PHX_ISLAND_SINGLE = 0, PHX_ISLAND_MULTIPLE = 1, PHX_ISLAND_SINGLE_SLOPPY = 2, PHX_ISLAND_MULTIPLE_SLOPPY = 3 };

/* ref: src/Configuration.h:20-23.  On this backend the wavefront is the SIMD unit, so solve_mode
 * does not select a code path: every mode runs per-joint (scalar, N=1) skip semantics in the
 * device's own colour order.  island_mode picks the schedule:
 *   Single                      one coupled system (one group), solved class by class out of HBM;
 *   Multiple, Single Sloppy,    the island-aware schedule: connected components (GatherIslands semantics) binned
 *   Multiple Sloppy             into workgroup-sized groups solved out of LDS, each with its own early exit and its
 *                               own copy of the static bodies' tags; components too big for a workgroup go to one
 *                               trailing group solved out of HBM.
 * The reference's Sloppy modes promise no order (racy 512-joint batches, ref: src/Solver.cpp:138-139); here
 * they run that deterministic island-aware schedule — a legal outcome of those modes.  islandCount /
 * islandMaxSize are published only by the two Multiple modes (1 / joint count otherwise), like the reference. */
typedef struct {
    int32_t solve_mode;
    int32_t island_mode;
    int32_t contact_iterations;
    int32_t penetration_iterations;
} phx_config;

/* byte-exact POD records (static_asserted in the implementation) */
typedef struct { float x, y; } phx_vec2;
typedef struct {                                  /* ref: src/RigidBody.h:12-57 */
    uint32_t index;
    phx_vec2 geom_size, geom_xvector, geom_yvector, geom_pos, aabb_min, aabb_max;
    phx_vec2 velocity, acceleration, displacing_velocity;
    float    angular_velocity, angular_acceleration, displacing_angular_velocity;
    float    inv_mass, inv_inertia;
    phx_vec2 xvector, yvector, pos;
    int32_t  last_iteration, last_displacement_iteration;
} phx_rigid_body;                                 /* 128 B */
typedef struct {                                  /* ref: src/Manifold.h:12-43 */
    phx_vec2 delta1, delta2, normal;
    uint8_t  is_merged, is_newly_created, pad_[2];
    int32_t  solver_index;
} phx_contact_point;                              /* 32 B */
typedef struct { int32_t body1, body2, point_count, point_index; } phx_manifold;   /* ref: src/Manifold.h:45-67, 16 B */
typedef struct {                                  /* ref: src/Joints.h:6-23 */
    int32_t contact_point_index, body1, body2;
    float   normal_accumulated_impulse, friction_accumulated_impulse;
} phx_contact_joint;                              /* 20 B */
typedef struct { float minx, maxx, centery, extenty; uint32_t index; } phx_broadphase_entry; /* ref: src/Collider.h:45-50, 20 B */
typedef struct { uint32_t value, index; } phx_sort_entry;                                     /* ref: src/Collider.h:52-56, 8 B  */

/* ---------------------------------------------------------------------------------------------- */
/* library                                                                                         */
int          phx_abi_version(void);
/* The arithmetic of the sweeps (PreStepJoints, SolveJointsImpulses, SolveJointsDisplacement; ref: src/Solver.cpp:697-1018), fixed
 * when the library is built.  The reference writes `dV -= projector * velocity` / `velocity += compMass * dImpulse` and ships
 * -ffast-math -mfma (ref: Makefile:11, 17-24), which leaves fusing those pairs to its compiler; this backend states it:
 *   PHX_ARITH_FUSED   every such multiply-add pair is one fused multiply-add (fmaf), in the reference's source order — the default;
 *   PHX_ARITH_SOURCE  a rounded product and a rounded sum, as the source spells it (`PHX_ARITH=source python -m phyx_amd.build`).
 * RefreshJoints and everything outside the sweeps is source order in both.  oracle/ has both forms; parity is bit-exact against
 * the matching one, and the two forms stay within SURVEY.md section 8(c)'s tolerances of each other (tests/test_arith_modes.py). */
enum { PHX_ARITH_SOURCE = 0, PHX_ARITH_FUSED = 1 };
int          phx_arith_mode(void);
const char*  phx_last_error(void);
int          phx_device_count(void);              /* >=0, or a negative phx_status */
/* name / CU count / LDS per workgroup of `device`; name_cap bytes incl. NUL */
int          phx_device_info(int device, char* name, int name_cap, int* compute_units, int* lds_bytes, int64_t* hbm_bytes);

/* ---------------------------------------------------------------------------------------------- */
/* Solver — replaces Solver::SolveJoints (ref: src/Solver.h:54, src/Solver.cpp:17-119)             */
typedef struct phx_solver phx_solver;

int  phx_solver_create(phx_solver** out, int device);
void phx_solver_destroy(phx_solver* s);

/* Drop-in for Solver::SolveJoints: HOST arrays in the reference's layouts.  Reads per body
 * invMass/invInertia/coords.pos and the four velocity fields, per contact point delta1/delta2/
 * normal, per joint indices + accumulated impulses; writes back bodies[i].velocity /
 * angularVelocity / displacingVelocity / displacingAngularVelocity (ref: Solver.cpp:488-492) and
 * the joints' two accumulated impulses (ref: Solver.cpp:543-544).  Uploads, solves on the device,
 * downloads — the PCIe cost is part of this call. */
int phx_solver_solve(phx_solver* s, phx_rigid_body* bodies, int32_t body_count,
                     const phx_contact_point* contact_points, int32_t contact_point_count,
                     phx_contact_joint* joints, int32_t joint_count, const phx_config* config);

/* Same computation on DEVICE-resident records (same layouts, HBM pointers), asynchronous on the
 * solver's stream; nothing crosses PCIe except the solve's control word.  The records are converted to the
 * resident arrays below and back around the solve (two extra passes over the bodies): the drop-in for a caller
 * that keeps the reference's RigidBody array in HBM. */
int phx_solver_solve_device(phx_solver* s, void* d_bodies, int32_t body_count,
                            const void* d_contact_points, int32_t contact_point_count,
                            void* d_joints, int32_t joint_count, const phx_config* config);
int phx_solver_synchronize(phx_solver* s);

/* The RESIDENT form of body state (north star: "bodies ... laid out SoA in HBM with coalesced loads").  The reference stages
 * exactly these fields into solver-side arrays on every call (PrepareBodies / FinishBodies, ref: src/Solver.cpp:456-494:
 * SolveBody {velocity, angularVelocity, lastIteration}, SolveBodyParams {invMass, invInertia, coords}); here the staged form is
 * what a resident pipeline KEEPS — this library's World does, and bench.py times this entry point — three device arrays of one
 * 16-byte granule per body:
 *   vel[b]  = {velocity.x, velocity.y, angularVelocity, 0}                        read + written in place
 *   dvel[b] = {displacingVelocity.x, .y, displacingAngularVelocity, 0}            read + written in place
 *   mpos[b] = {invMass, invInertia, pos.x, pos.y}                                 read only
 * phx_bodies_to_view / phx_view_to_bodies convert between a device array of records and a view (queued on `stream`, a
 * hipStream_t, e.g. phx_solver_stream; the second writes the four velocity fields only, like FinishBodies). */
typedef struct { void* vel; void* dvel; void* mpos; } phx_body_view;
int phx_solver_solve_resident(phx_solver* s, const phx_body_view* bodies, int32_t body_count,
                              const void* d_contact_points, int32_t contact_point_count,
                              void* d_joints, int32_t joint_count, const phx_config* config);
int phx_bodies_to_view(int device, const void* d_bodies, int32_t body_count, const phx_body_view* out, void* stream);
int phx_view_to_bodies(int device, const phx_body_view* in, int32_t body_count, void* d_bodies, void* stream);

/* Precision ablation (BASELINE config 5): 32 (default) keeps the solver-side body state {velocity, angular velocity}
 * in fp32 like the reference's SolveBody (ref: src/Solver.h:95-101); 16 stores it as IEEE half between joint updates
 * (arithmetic stays fp32, every store rounds to nearest-even) in the groups solved out of LDS.  Not a drop-in mode:
 * results differ from the reference's by the rounding; tests compare against an oracle that rounds the same way. */
int phx_solver_set_body_state_bits(phx_solver* s, int32_t bits);

/* Island sharding across ranks: the schedule's groups (phx_solver_get_groups) are body-disjoint, so rank `shard` of
 * `shard_count` sweeps only the groups it owns (phx_exchange_layout's deal: longest processing time first by joint count;
 * the trailing HBM group counts as group lds_count) and leaves every other body and joint untouched.  All ranks must be given the same joints; the union of
 * their results is the unsharded result, bit for bit.  Default 0 / 1 = everything. */
int phx_solver_set_shard(phx_solver* s, int32_t shard, int32_t shard_count);

/* 1 (default): a solve whose joint topology fingerprint matches the cached schedule reuses it (checked on the device,
 * see DESIGN.md §4.1).  0: every solve rebuilds its schedule, like the reference rebuilds PrepareIndices / GatherIslands on
 * every call (ref: src/Solver.cpp:77, 135) — the cost a world whose contact graph changes every step pays. */
int phx_solver_set_schedule_reuse(phx_solver* s, int32_t on);

/* Diagnostics: with tracing on, every workgroup of the island kernel stamps the 100 MHz wall clock at its phase boundaries.
 * phx_solver_get_island_trace copies 8 words per LDS group of the last solve: [0] start, [1] records loaded, [2] refreshed,
 * [3] pre-stepped, [4] swept, [5] written back, [6] XCC id, [7] colours << 32 | impulse sweeps executed.  *groups receives
 * the group count (out may be NULL to query it).  on: 0 = off, 1 = the phase stamps only (a few stores per workgroup: the kernel
 * keeps its speed), any other value = also the per-wave cycle counts of every class step (phx_solver_get_wave_trace; ~15 % slower). */
int phx_solver_set_trace(phx_solver* s, int32_t on);
int phx_solver_get_island_trace(phx_solver* s, uint64_t* out, int32_t cap_groups, int32_t* groups);
/* per wave of every LDS group (groups x *waves_per_group x 8 words): shader cycles spent in colour steps in which the wave
 * worked {[0] in the joint update with at most 32 lanes active, [1] at the barrier behind it}, [2] cycles of the steps it only
 * waited in, [3] working steps with at most 32 lanes << 32 | idle steps, [4] cycles in the joint update with more than 32
 * lanes active, [5] such steps */
int phx_solver_get_wave_trace(phx_solver* s, uint64_t* out, int32_t cap_words, int32_t* waves_per_group);
/* per LDS group (groups x *words_per_group words), the 100 MHz clock: [0] the first level of the set-up's loads is back, [1] the second,
 * [2] records in LDS and compared, [3] refreshed, [4..7] PreStep classes 0..3 done, [8] first sweep done, [9] commit decided,
 * [10] results issued; [16 + 8 w ...] wave w, summed over its working class steps of the impulse-only sweeps, in shader cycles (filled
 * with the per-wave counts on only): barrier released -> LDS data back, -> last FMA, -> stores issued, -> LDS acknowledged, -> barrier
 * released, [5] such steps (only those in which the wave's first lane was evaluated are counted: the intervals are that lane's), [6] 1 if the wave touches a static body */
int phx_solver_get_phase_trace(phx_solver* s, uint64_t* out, int32_t cap_words, int32_t* words_per_group);

/* Post-solve exchange of an island-sharded solve (BASELINE config 3; counterpart of the reference merging every island's
 * bodies back after its parallel island loop, ref: src/Solver.cpp:86-91, 482-494, 527-547).  Every rank holds a replica
 * of the inputs and solves only its own groups; afterwards
 *   phx_solver_exchange_pack     queues kernels that pack this rank's results (6 floats per body, 2 per joint of its
 *                                groups, behind a 32-byte header) into the send buffer and returns the segment size —
 *                                the same on every rank, because the layout is a pure function of the schedule;
 *   the CALLER all-gathers       segment_bytes from every rank's send buffer into the recv buffer (rank r at byte offset
 *                                r * segment_bytes) on phx_solver_stream() — RCCL over xGMI on a GPU node;
 *   phx_solver_exchange_unpack   queues kernels that scatter the other ranks' results into this rank's arrays and check
 *                                every peer's header (step serial, status word, topology fingerprint).
 * After the unpack all replicas are bit-identical to the unsharded solve.  Buffers are caller-owned device memory
 * (16-byte aligned; recv holds shard_count segments of segment_capacity_bytes, a multiple of 256).  status_word != 0 in
 * pack tells the peers that this rank failed earlier in the step.  phx_solver_exchange_status synchronises and returns
 * the OR of PHX_XCH_* bits seen by the unpacks so far (0 = every exchange was consistent). */
enum { PHX_XCH_PEER_ERROR = 1, PHX_XCH_SERIAL_MISMATCH = 2, PHX_XCH_TOPOLOGY_MISMATCH = 4, PHX_XCH_BAD_SEGMENT = 8 };
int    phx_solver_set_exchange_buffers(phx_solver* s, void* d_send, void* d_recv, size_t segment_capacity_bytes);
int    phx_solver_exchange_pack(phx_solver* s, const void* d_bodies, const void* d_joints, int32_t status_word, size_t* segment_bytes);
int    phx_solver_exchange_unpack(phx_solver* s, void* d_bodies, void* d_joints);
int    phx_solver_exchange_status(phx_solver* s, int32_t* status);
size_t phx_solver_exchange_segment_bytes(phx_solver* s);      /* of the last pack */
/* Host-only: who solves what, and the segment layout.  The groups (body table of group_bodies[g] entries, group_slots[g] joints)
 * are dealt to the ranks longest-processing-time first: by decreasing joint count (ties: group number), each to the rank with
 * the fewest joints so far (ties: lowest rank) — round-robin on uniform columns, balanced on anything else; group_owner[g] = that
 * rank.  group_offset_words[g] = 32-bit word offset of the group's block inside its owner's segment (a rank's groups in ascending
 * group order), rank_words[r] = words rank r actually fills (all three optional), *segment_words = the common padded length. */
int    phx_exchange_layout(const int32_t* group_bodies, const int32_t* group_slots, int32_t group_count, int32_t shard_count,
                           int32_t* group_owner, int64_t* group_offset_words, int64_t* rank_words, int64_t* segment_words);

/* ---------------------------------------------------------------------------------------------- */
/* Native transport of the island-sharded solve: an RCCL communicator, one process per GPU (xGMI between them).  The        */
/* reference's islands are solved by threads of one process and merged in its one address space (ref: src/Solver.cpp:86-91, */
/* 482-494, 527-547); across GPUs that merge is one all-gather per step on the solver's stream, which is also the per-step   */
/* barrier.  RCCL is resolved at run time (librccl.so.1; PHX_RCCL_LIB overrides): no link dependency, PHX_ERR_NO_DEVICE when */
/* it cannot be loaded.  Rendezvous is the caller's: rank 0 calls phx_comm_unique_id and hands the PHX_COMM_ID_BYTES bytes   */
/* to every rank by any out-of-band channel (a file, a socket, MPI, torch.distributed's store), then every rank creates.    */
#define PHX_COMM_ID_BYTES 128
typedef struct phx_comm phx_comm;
int  phx_comm_unique_id(void* out_id);                                  /* ncclGetUniqueId */
/* ncclCommInitRank (collective).  A rank whose peers do not arrive within PHX_COMM_TIMEOUT_S seconds (environment, default 120) gives */
/* up with PHX_ERR_STATE instead of hanging; the same bound holds wherever this library blocks the host on a collective.            */
int  phx_comm_create(phx_comm** out, const void* unique_id, int32_t rank, int32_t nranks, int device);
void phx_comm_destroy(phx_comm* c);
int  phx_comm_rccl_version(void);                                       /* ncclGetVersion of the RCCL in use, 0 if none could be loaded */
int  phx_comm_rank(phx_comm* c);
int  phx_comm_size(phx_comm* c);
/* bytes_per_rank from every rank's d_send into d_recv (rank r at r * bytes_per_rank), queued on `stream` (a hipStream_t) */
int  phx_comm_all_gather(phx_comm* c, const void* d_send, void* d_recv, size_t bytes_per_rank, void* stream);
int  phx_comm_barrier(phx_comm* c, void* stream);                       /* 4-byte all-reduce + stream wait: the pure barrier */
int  phx_comm_barrier_async(phx_comm* c, void* stream);                 /* the same all-reduce, only queued: work queued on `stream` behind it waits for every rank */
int  phx_comm_async_error(phx_comm* c, int32_t* error);                 /* ncclCommGetAsyncError: 0 = healthy */
/* attach to a solver: phx_solver_bench then runs pack -> all-gather -> unpack natively in every step (exchange buffers must be set) */
int  phx_solver_set_comm(phx_solver* s, phx_comm* c);

/* results of the last solve (valid after a synchronizing call) — counterparts of
 * Solver::islandCount / islandMaxSize (ref: src/Solver.h:105-106) plus executed sweep counts */
typedef struct {
    int32_t island_count, island_max_size;
    int32_t colour_count;
    int32_t impulse_iterations;        /* sweeps executed before the no-productive-joint exit (ref: Solver.cpp:189) */
    int32_t displacement_iterations;   /* ref: Solver.cpp:210 */
    int32_t lds_islands;               /* islands solved by the one-workgroup-per-island kernel */
    int32_t recoloured;                /* 1 if the joint topology changed and the schedule was rebuilt; 2 if that rebuild ran without a host
                                          round trip (bins made on the device with last build's bin count as the launch grid) */
    int32_t graph_replay;              /* always 0: the launch sequence is never replayed from captured graphs (kept for the layout) */
    double  device_ms;                 /* HIP-event time of the device work of the last solve */
    int64_t joint_visits;              /* joints swept by the impulse loop, skipped ones included; per-island early exits honoured */
} phx_solve_stats;
int phx_solver_get_stats(phx_solver* s, phx_solve_stats* out);

/* The schedule the device used: order[k] = index of the joint occupying slot k; colour (class) c owns slots
 * [colour_offsets[c], colour_offsets[c+1]).  Sweeping the slots front to back with the reference's
 * scalar loop reproduces the device result bit for bit (tests/ feeds this to the oracle).
 * A class is a set of UNITS that share no dynamic body; a unit is the one or two joints of a body pair (the
 * two contact points of a manifold).  Its slots are laid out as: the leaders that have a follower (joint
 * order), the single leaders (joint order), then the followers in their leaders' order — a lane of the
 * device sweeps a leader and then its follower on one read and one write of the two bodies. */
int phx_solver_get_schedule(phx_solver* s, int32_t* order, int32_t order_cap,
                            int32_t* colour_offsets, int32_t offsets_cap, int32_t* colour_count);
/* Groups of the schedule: group g owns slots [group_offsets[g], group_offsets[g+1]) and is an independent
 * Gauss-Seidel problem (body-disjoint from every other group, static bodies aside) with its own early exit and
 * its own copy of the static bodies' lastIteration tags — the counterpart of the reference's islands
 * (ref: Solver.cpp:86-91).  The first *lds_group_count groups ran one-workgroup-per-group out of LDS, the rest
 * (at most one) class by class out of HBM.  Single island mode always reports one group. */
int phx_solver_get_groups(phx_solver* s, int32_t* group_offsets, int32_t offsets_cap, int32_t* group_count, int32_t* lds_group_count);

/* Partitioned components: a connected component of more than 1024 joints — a settled pile — has its units
 * split into INTERIOR ones (both bodies dynamic and in the same block of 512 consecutive body indices: level 0; or, failing that,
 * in the same block of that grid shifted by 256: level 1) and the rest; the interior units occupy the first `interior_classes`
 * classes of the schedule's last group (level 0 before level 1) and are swept by ONE launch per level and sweep (a workgroup per
 * block, `parts` of them over both levels; 0 when the schedule has no such component or PHX_NO_PARTS=1).  `sweep_launches`:
 * kernel launches of the last solve's sweeps. */
int phx_solver_get_partition(phx_solver* s, int32_t* interior_classes, int32_t* parts, int32_t* sweep_launches);
/* The lanes the island kernel gave the units of the last solve's LDS groups (execution detail, for tests and diagnostics: the classes'
 * lane ranges are placed on wave boundaries where the lanes allow it, see phx_schedule_groups): per unit the slot of its leader in
 * phx_solver_get_schedule's order and its lane inside its group's workgroup; *count = units (pass NULL arrays to ask for it). */
int phx_solver_get_lanes(phx_solver* s, int32_t* leader_slot, int32_t* lane, int32_t cap, int32_t* count);

/* RefreshJoints output for joint `joint_index` of the last solve (ref: Solver.cpp:592-695), expanded
 * to the reference's 30-float ContactJointPacked<1> order: normal limiter 13, 0, dstVelocity,
 * dstDisplacingVelocity, accumulatedDisplacingImpulse(after solve), friction limiter 13. */
int phx_solver_get_refreshed(phx_solver* s, int32_t joint_index, float out30[30]);

/* Host-only schedule builders (no device needed) — exposed so the ordering logic can be checked on
 * its own.  phx_schedule_colours is this backend's counterpart of Solver::PrepareIndices
 * (ref: src/Solver.cpp:217-273).  Joints are first paired into units: two joints whose priority ids
 * differ in the lowest bit only (contact points 2m and 2m + 1 of manifold m) and whose bodies are the
 * same form a unit, led by the even id; every other joint is a unit of its own.  The units are
 * partitioned into classes that share no dynamic body (is_static[b] != 0 exempts body b): they take
 * their class first-fit in order of DECREASING phx_schedule_priority(priority_ids[j], j, min(body1[j],
 * body2[j])) of their leader j — units whose lower body index is even first, inside a parity a fixed
 * pseudo-random order: the device reaches the same classes in a few parallel rounds (two on a stacked
 * column), whereas joint-index order needs one round per box of a stacked column — with
 * two candidates per connected component (smallest free class / two-ended) of which the component keeps
 * the one that needs fewer classes.  The layout of a class is described at phx_solver_get_schedule.
 * priority_ids may be NULL (the joint index is used); the solver passes each joint's
 * contactPointIndex, which survives compaction of the joint list (island sharding).
 * phx_schedule_islands follows Solver::GatherIslands (ref: src/Solver.cpp:285-454):
 * joint_island[j] = coalesced island of joint j (-1 if both bodies are static), island_size[i] =
 * joints in island i; returns the island count. */
int phx_schedule_colours(const int32_t* body1, const int32_t* body2, int32_t joint_count,
                         const uint8_t* is_static, int32_t body_count, const int32_t* priority_ids,
                         int32_t* order, int32_t* colour_offsets, int32_t offsets_cap, int32_t* colour_count);
int phx_schedule_islands(const int32_t* body1, const int32_t* body2, int32_t joint_count,
                         const uint8_t* is_static, int32_t body_count,
                         int32_t* joint_island, int32_t* island_size, int32_t island_cap);
/* Host-only: the island-mode schedule (ref: Solver.cpp:285-454 GatherIslands + :217-273 PrepareIndices) as the workgroup-sized groups
 * this backend solves out of LDS: connected components binned into groups of at most `lanes` units / 2 * lanes joints / body_cap
 * bodies (whatever does not fit goes to one trailing group); the classes of a group are coloured like phx_schedule_colours colours a
 * component.  order / colour_offsets as there; group_offsets (slots) and group_first_colour have groups + 1 entries, *lds_groups of
 * the groups are LDS groups; per unit of the LDS groups (class-major, group by group; the return value is their number): the slot of
 * its leader and its lane in the island kernel — the classes' lane ranges are placed on wave boundaries where the lanes allow it
 * (a class costs one pass of every wave it has a lane in); lanes are execution detail, no result depends on them. */
int phx_schedule_groups(const int32_t* body1, const int32_t* body2, int32_t joint_count, const uint8_t* is_static, int32_t body_count,
                        const int32_t* priority_ids, int32_t lanes, int32_t body_cap, int32_t* order, int32_t* colour_offsets,
                        int32_t offsets_cap, int32_t* colour_count, int32_t* group_offsets, int32_t* group_first_colour,
                        int32_t groups_cap, int32_t* lds_groups, int32_t* unit_lane, int32_t* unit_leader_slot);
uint64_t phx_schedule_priority(uint32_t priority_id, uint32_t joint_index, uint32_t lower_body);

/* ---------------------------------------------------------------------------------------------- */
/* Broadphase — replaces Collider::UpdateBroadphase + UpdatePairs                                   */
/* (ref: src/Collider.h:28-29, src/Collider.cpp:251-366, src/base/RadixSort.h:19-95)               */
typedef struct phx_broadphase phx_broadphase;

int  phx_broadphase_create(phx_broadphase** out, int device);
void phx_broadphase_destroy(phx_broadphase* b);
/* forget every persistent pair (ref: main.cpp:88 manifoldMap.clear()) */
int  phx_broadphase_clear(phx_broadphase* b);

/* UpdateBroadphase + UpdatePairs on HOST bodies (reads geom.aabb only).  new_pairs receives the
 * pairs that were not yet in the persistent pair set, as (index_i, index_j) in the reference's
 * serial emission order (ref: Collider.cpp:296-318), and inserts them into the set.
 * *new_pair_count always receives the full count (PHX_ERR_CAPACITY if it exceeds the cap). */
int phx_broadphase_update(phx_broadphase* b, const phx_rigid_body* bodies, int32_t body_count,
                          uint32_t* new_pairs, int32_t new_pairs_cap, int32_t* new_pair_count);
int phx_broadphase_update_device(phx_broadphase* b, const void* d_bodies, int32_t body_count);
/* after an update: broadphaseSort[1] and broadphase[] of the reference (ref: Collider.h:64-65) */
int phx_broadphase_get_sorted(phx_broadphase* b, phx_sort_entry* sorted, phx_broadphase_entry* entries, int32_t cap);
/* pairs emitted by the last update (device variant leaves them on the device until asked) */
int phx_broadphase_get_new_pairs(phx_broadphase* b, uint32_t* new_pairs, int32_t cap, int32_t* count);
/* remove pairs from the persistent set (ref: Collider.cpp:391 manifoldMap.erase) */
int phx_broadphase_erase_pairs(phx_broadphase* b, const uint32_t* pairs, int32_t pair_count);
typedef struct {
    int64_t candidate_tests;      /* y-overlap tests executed by the sweep (20 B each) */
    int64_t overlapping_pairs;    /* candidates that passed the y test                               */
    int32_t new_pairs;
    int32_t set_size;             /* persistent pairs after the update                               */
    double  device_ms;
} phx_broadphase_stats;
int phx_broadphase_get_stats(phx_broadphase* b, phx_broadphase_stats* out);

/* ---------------------------------------------------------------------------------------------- */
/* World — replaces World (ref: src/World.h:9-36, src/World.cpp:11-37)                              */
typedef struct phx_world phx_world;

int  phx_world_create(phx_world** out, int device);
void phx_world_destroy(phx_world* w);
/* World::AddBody (ref: World.cpp:11-17; RigidBody ctor RigidBody.h:15-36, density 1e-5); returns index */
int  phx_world_add_body(phx_world* w, float px, float py, float angle, float half_x, float half_y);
/* main.cpp:91-93 groundBody->invMass = invInertia = 0 */
int  phx_world_set_body_static(phx_world* w, int32_t body);
/* body->invMass = ..., body->invInertia = ... on a public RigidBody (the demo scenes pin shelves with invMass = 0 only, so they
 * still rotate: main.cpp:176-177, 194-195; a body is static — exempt from islands — only when both are 0, ref: Solver.cpp:304) */
int  phx_world_set_body_inverse_mass(phx_world* w, int32_t body, float inv_mass, float inv_inertia);
int  phx_world_set_gravity(phx_world* w, float gravity);            /* ref: World.h:35 */
/* Multi-GPU island sharding: every rank steps a replica of the same world and solves only the schedule groups g with
 * g % shard_count == shard (phx_solver_set_shard; the default 0/1 solves everything).  A sharded world (shard_count > 1)
 * steps in two halves around the caller's all-gather (see phx_solver_exchange_pack; the buffers are set on
 * phx_world_solver(w) with phx_solver_set_exchange_buffers):
 *   phx_world_step_begin   World::Update up to and including SolveJoints of this rank's groups, then the pack;
 *   all-gather             of *segment_bytes per rank, send buffer -> recv buffer, on phx_world_stream(w);
 *   phx_world_step_end     scatter of the other ranks' results, then IntegratePosition.
 * phx_world_update / phx_world_finish_step refuse to run on a sharded world (PHX_ERR_STATE): without the exchange they
 * would integrate the other ranks' bodies with unsolved velocities. */
int  phx_world_set_shard(phx_world* w, int32_t shard, int32_t shard_count);
int  phx_world_step_begin(phx_world* w, float dt, const phx_config* config, size_t* segment_bytes);
int  phx_world_step_end(phx_world* w, float dt);
void* phx_world_stream(phx_world* w);       /* the hipStream_t all of the world's work is queued on */
/* The same step with the native transport: phx_world_set_comm makes this world rank phx_comm_rank(c) of phx_comm_size(c)
 * (the world owns and grows its exchange buffers), and phx_world_step_sharded is World::Update of the sharded world in ONE
 * call — step_begin, ncclAllGather of the segments on the world's stream, step_end — with no host wait around the collective.
 * Every 16th step (and on phx_world_check_exchange) the peers' headers and ncclCommGetAsyncError are checked: PHX_ERR_STATE
 * means a peer failed, is at another step or solved another topology (phx_solver_exchange_status has the bits). */
int  phx_world_set_comm(phx_world* w, phx_comm* c);
int  phx_world_step_sharded(phx_world* w, float dt, const phx_config* config);
int  phx_world_check_exchange(phx_world* w);
int  phx_world_update(phx_world* w, float dt, const phx_config* config);   /* ref: World.cpp:19-37 */
/* phx_world_update returns once the step is QUEUED on the world's stream (the host waits only where it needs a count
 * to size a launch); every getter synchronises before it reads.  This waits for the device explicitly. */
int  phx_world_synchronize(phx_world* w);
/* World::Update split at the solver boundary: pre_solve = everything before Solver::SolveJoints
 * (ref: World.cpp:25-32), after which bodies / contact points / joints are exactly the solver's inputs;
 * finish_step = SolveJoints + IntegratePosition (ref: World.cpp:34-36).  pre_solve + finish_step == update. */
int  phx_world_pre_solve(phx_world* w, float dt);
int  phx_world_finish_step(phx_world* w, float dt, const phx_config* config);
int  phx_world_counts(phx_world* w, int32_t* bodies, int32_t* manifolds, int32_t* contact_points, int32_t* joints);
int  phx_world_get_bodies(phx_world* w, phx_rigid_body* out, int32_t cap);
int  phx_world_get_manifolds(phx_world* w, phx_manifold* out, int32_t cap);
int  phx_world_get_contact_points(phx_world* w, phx_contact_point* out, int32_t cap);
int  phx_world_get_joints(phx_world* w, phx_contact_joint* out, int32_t cap);
/* EDITS BETWEEN STEPS — what the reference's application does to its public RigidBody array before every Update (ref: main.cpp:337-349,
 * the mouse drag; RigidBody.h:38-42).  Every edit is a batch: `count` body indices with their values, read from host memory.
 *   - Queued on phx_world_stream(w) behind whatever is queued there; the call returns as soon as the caller's arrays may be reused
 *     (they are staged through pinned memory the world owns) and does not wait for a step still in flight.
 *   - Between steps only: an edit made between phx_world_pre_solve and phx_world_finish_step, or between phx_world_step_begin and
 *     phx_world_step_end, returns PHX_ERR_STATE.
 *   - Checked completely before anything is queued: count >= 0, every index in [0, body count), no index twice in one call;
 *     PHX_ERR_INVALID otherwise, and the world is unchanged.  Edits of separate calls apply in call order.
 *   - An edit of host-staged bodies (before the first step, or after add_body / set_body_static / set_body_inverse_mass) acts as if
 *     written into their records; edits queued on the device survive a later host-staging call.
 *   - They change no joint topology: the cached solver schedule stays valid.
 *   - Sharded worlds: in replica mode (phx_world_set_shard / set_comm) every rank must apply the same batches, as with every other
 *     input.  The indices are the world's own; an ownership-sharded (slab) world's indices are local to its rank.
 * acceleration += {ax, ay}, angularAcceleration += angular (ref: main.cpp:343-346), accel = 3 floats per body.  They add to whatever is
 * pending (accelerations restored by phx_world_set_state included), show in the records until the next step's IntegrateVelocity
 * consumes them (ref: World.cpp:44-53), and read as zero after it. */
int  phx_world_add_accelerations(phx_world* w, const int32_t* bodies, const float* accel, int32_t count);
/* velocity = {vx, vy}, angularVelocity = angular; vel = 3 floats per body */
int  phx_world_set_velocities(phx_world* w, const int32_t* bodies, const float* vel, int32_t count);
/* coords = {pos, xVector, yVector}, then UpdateGeom (ref: RigidBody.h:38-42, Geom.h:79-85): the AABB is recomputed, and the next step's
 * broadphase and UpdateManifolds see the new geometry.  pose = 6 floats per body {pos.x, pos.y, xv.x, xv.y, yv.x, yv.y}: a frame,
 * not an angle, so that nothing is rounded on the way (phyx_amd.World.set_poses builds frames from angles as add_body does). */
int  phx_world_set_poses(phx_world* w, const int32_t* bodies, const float* pose, int32_t count);
/* GATHERS (any time, like phx_world_get_bodies; they wait for the queued work).  The 128-byte records of the listed bodies,
 * byte-equal to phx_world_get_bodies()[bodies[k]]; O(count) work and transfer.  Indices as above, repeats allowed. */
int  phx_world_get_body_states(phx_world* w, const int32_t* bodies, int32_t count, phx_rigid_body* out);
/* {pos.x, pos.y, xVector.x, xVector.y} of every body, 16 B per body (cap: room for that many bodies, PHX_ERR_CAPACITY otherwise) */
int  phx_world_get_poses(phx_world* w, float* out, int32_t cap);
/* the same into caller-owned device memory (16-byte aligned), queued on phx_world_stream(w): no host wait, nothing over PCIe */
int  phx_world_get_poses_device(phx_world* w, void* d_out, int32_t cap);
/* REMOVAL BETWEEN STEPS.  Removing the set R of bodies leaves exactly the world phx_world_set_state would make of the filtered state
 * filter(bodies, manifolds, contact points, joints, R), where
 *   - bodies: the bodies not in R, in their old order; new[i] = the new index of old body i, or -1 if it was removed.  Each kept record
 *     is copied unchanged except `index`, which becomes its new position (ref: World.cpp:14); pending accelerations move with it;
 *   - manifolds: kept iff both bodies are kept, in their old order, body1 / body2 remapped through new[] (new[] is monotonic, so
 *     body1 < body2 still holds wherever it held), point_index = 2 * the manifold's new index;
 *   - contact points: the two slots of each kept manifold move with it; a live slot's (k < point_count) solver_index becomes its
 *     joint's new index (-1 if that joint goes; an index outside [0, joint count) stays as it is); dead slots are copied byte for byte;
 *   - joints: kept iff their manifold is kept (equivalently: both of their bodies are), in their old order, body1 / body2 remapped,
 *     contact_point_index = 2 * (the manifold's new index) + old % 2, warm-start impulses unchanged;
 *   - the broadphase's pair set becomes the kept manifolds' remapped pairs, and everything set_state resets is reset: the cached
 *     solver schedule is rebuilt at the next step.
 * Rules as for the edits above: between steps only (PHX_ERR_STATE inside pre_solve .. finish_step or step_begin .. step_end); a sharded
 * or communicator-attached world gets PHX_ERR_STATE, as set_state does; the arguments are checked completely before anything is
 * queued (every index in [0, body count), none twice; PHX_ERR_INVALID otherwise, the world unchanged).  Removing no body is a true
 * no-op (the cached schedule stays valid), removing every body is allowed.  Host-staged bodies (before the first step, after add_body /
 * set_body_static / set_body_inverse_mass) are uploaded first, as the next step would upload them.  The work runs on the world's
 * stream with one host round trip for the new counts; nothing of the state crosses PCIe but the remap, when asked for.
 * Every index the caller holds shifts: body i is now remap[i].  An ownership-sharded (slab) world's indices are local to its rank;
 * phyx_amd/dist.py SlabWorld's scene indices are not kept in step with a removal.
 * remap (may be NULL): room for the old body count; receives new[] (new index or -1). */
int  phx_world_remove_bodies(phx_world* w, const int32_t* bodies, int32_t count, int32_t* remap);
/* Remove every body whose AABB does not overlap the closed box {min.x, min.y, max.x, max.y} (the despawn rule: a kill plane, a play
 * area).  The test runs on the device over the resident AABBs: no positions cross PCIe.  Static bodies are not exempt.  The box must be
 * finite with min <= max (PHX_ERR_INVALID otherwise).  *removed (may be NULL) = how many went; remap as above.  When every body is
 * inside, nothing changes. */
int  phx_world_remove_outside(phx_world* w, const float box[4], int32_t* removed, int32_t* remap);
/* SPAWN BETWEEN STEPS.  Appends `count` bodies; body first + k is byte for byte the record the k-th of `count` calls of
 * phx_world_add_body(px, py, angle, half_x, half_y) would have made (index = its position).  spawn = 5 floats per body
 * {px, py, angle, half_x, half_y}; *first (may be NULL) receives the index of the first new body.
 * Rules as for the edits and the removal above: between steps only (PHX_ERR_STATE); a sharded or communicator-attached world gets
 * PHX_ERR_STATE; checked completely before anything is queued (count >= 0, no NULL array when count > 0, every value finite, both half
 * extents > 0, the new body count within int32; PHX_ERR_INVALID otherwise, the world unchanged); an empty call is a true no-op.
 * Before the first step (host-staged bodies) it is exactly `count` phx_world_add_body calls.  After a step it is queued on
 * phx_world_stream(w) and returns once `spawn` may be reused: the frame is built on the host as add_body builds it, 40 bytes per body
 * cross PCIe, and one kernel writes the records and the resident state.  Nothing of the existing world crosses PCIe, and it waits for a
 * step in flight only where a body buffer has to grow (geometrically, keeping its contents).  The spawned bodies belong to no joint:
 * the cached solver schedule and the broadphase's splitters stay in use. */
int  phx_world_add_bodies(phx_world* w, const float* spawn, int32_t count, int32_t* first);
/* the batch form of phx_world_set_body_inverse_mass: values = {inv_mass, inv_inertia} per body (0, 0 = static).  Rules as for the
 * edits above (indices in range and distinct; values finite and >= 0), except that it changes the joint topology as the single form
 * does: the static set is part of the solver's schedule, which is rebuilt at the next step. */
int  phx_world_set_inverse_masses(phx_world* w, const int32_t* bodies, const float* values, int32_t count);
/* COLLISION FILTERS — which bodies collide at all.  Every body has a filter {category, mask, group}; the default {1, 0xFFFFFFFF, 0}
 * lets every pair through, and a world whose filters are all the default steps exactly as one that never heard of filters.
 *   - Rule: the pair (a, b) may collide iff
 *       a.group == b.group && a.group != 0:  group > 0 (a shared positive group always collides, a shared negative group never);
 *       otherwise:                           (a.mask & b.category) != 0 && (b.mask & a.category) != 0.
 *     Static bodies are filtered like any other body: a body whose mask excludes the ground's category falls through it.
 *   - Where it acts: UpdatePairs (ref: Collider.cpp:296-366) does not emit a pair that fails it.  The pair never enters the
 *     broadphase's pair set, never gets a manifold, contact points or joints, and the contact reports never see it.
 *     phx_broadphase_stats keeps its meaning: candidate_tests and overlapping_pairs count before the filter, new_pairs what was emitted.
 *   - Setting filters: the rules of the edits above.  Between steps only (PHX_ERR_STATE); checked completely before anything is queued
 *     (count >= 0, no NULL array when count > 0, every index in [0, body count), none twice; PHX_ERR_INVALID otherwise, the world
 *     unchanged); staged through pinned memory and queued on phx_world_stream(w); before the first step it writes the host-staged
 *     bodies' filters.  A sharded or communicator-attached world gets PHX_ERR_STATE.
 *   - Pairs that exist already: a manifold whose pair fails the new filters is dropped, and the result is exactly what
 *     phx_world_set_state would make of drop(state): bodies unchanged; the remaining manifolds in their old order with point_index =
 *     2 * the new index; their contact-point slots move with them, a live slot's solver_index following its joint (-1 if the joint
 *     goes); the joints of dropped manifolds go, the others keep their order with contact_point_index = 2 * (the manifold's new index)
 *     + old % 2; the broadphase's pair set becomes the kept manifolds' pairs and the cached solver schedule is rebuilt at the next step.
 *     (The removal's compaction above, with "the pair passes" as its keep rule.)  *dropped (may be NULL) receives the number of
 *     manifolds dropped.  When none is, the call changes no topology: the cached schedule stays valid.  Dropped pairs leave the
 *     touching set, so the next phx_world_contact_events reports them under end; the filters themselves do not touch its baseline.
 *   - The other calls: add_body / add_bodies give new bodies the default filter; remove_bodies / remove_outside move filters with
 *     the kept bodies (through new[]); phx_world_set_state resets every filter to the default (a filtered world is checkpointed as
 *     set_state followed by set_collision_filters); set_inverse_masses, the edits, queries and contact reports leave them alone.
 *     Queries see every body whatever its filter.
 *   - Sharded worlds carry no filters: phx_world_set_shard (shard_count > 1), phx_world_set_comm (a communicator) and
 *     phx_world_reslab return PHX_ERR_STATE while some body's filter differs from the default.
 * The test runs on the device inside the broadphase's sweep, before the pair-set lookup: one 16-byte gather per y-overlapping
 * candidate, and only in a world where some filter was ever set (the sweep of any other world is the unfiltered code). */
typedef struct { uint32_t category, mask; int32_t group; } phx_collision_filter;     /* 12 B */
int  phx_world_set_collision_filters(phx_world* w, const int32_t* bodies, const phx_collision_filter* filters, int32_t count, int32_t* dropped);
/* every body's filter, in index order (cap: room for that many; PHX_ERR_CAPACITY otherwise) */
int  phx_world_get_collision_filters(phx_world* w, phx_collision_filter* out, int32_t cap);
/* COLLISION EXCLUSIONS — body pairs that never collide.  The world owns a set of unordered body pairs {a, b}, a != b: a setting, like
 * the filter column.  It says what the filters cannot: a chain's link i passes through links i - 1 and i + 1, which it overlaps at
 * the hinge, and still collides with every other link (a shared negative group is transitive, a chain's neighbour relation is not).
 * A world whose set is empty allocates and launches exactly what it did before there were exclusions.
 *   - Rule: a pair in the set is not emitted by UpdatePairs (ref: Collider.cpp:296-366).  It never enters the broadphase's pair set,
 *     never gets a manifold, contact points or joints, and the contact reports never see it.
 *   - Where it acts: inside the sweep, behind the collision filter and in front of the pair-set lookup.  phx_broadphase_stats keeps
 *     its meaning: candidate_tests and overlapping_pairs count before both tests, new_pairs what was emitted.  The drop-in
 *     phx_broadphase_* handles know no exclusions.
 *   - The set: a pair is stored as {lo, hi} = {min(a, b), max(a, b)}.  add is set union (a pair already present changes nothing),
 *     remove set difference (an absent pair is ignored), clear empties the set.  get writes the pairs ascending by (lo, hi), two
 *     int32 per pair; it always fills *count (may be NULL) and returns PHX_ERR_CAPACITY if cap (in pairs) is smaller.
 *   - Checks: the rules of the edits above.  Between steps only (PHX_ERR_STATE); checked completely before anything is queued
 *     (count >= 0, no NULL array when count > 0, both indices of every pair in [0, body count), a != b, no pair twice in one call —
 *     (a, b) and (b, a) are the same pair; PHX_ERR_INVALID otherwise, phx_last_error names the first failure, the world unchanged).
 *     An empty call is a true no-op.  A sharded or communicator-attached world gets PHX_ERR_STATE.  Before the first step the set
 *     waits on the host with the host-staged bodies, as pins do.
 *   - Pairs that exist already: add drops the manifolds whose pair is now excluded, and the result is exactly what
 *     phx_world_set_state would make of drop(state): bodies unchanged; the remaining manifolds in their old order with point_index =
 *     2 * the new index; their contact-point slots move with them, a live slot's solver_index following its joint (-1 if the joint
 *     goes); the joints of dropped manifolds go, the others keep their order with contact_point_index = 2 * (the manifold's new index)
 *     + old % 2; the broadphase's pair set becomes the kept manifolds' pairs and the cached solver schedule is rebuilt at the next step.
 *     (The compaction COLLISION FILTERS describes, with "the pair is not in the set" as its keep rule.)  *dropped (may be NULL) receives
 *     the number of manifolds dropped.  When none is, the call changes no topology: the cached schedule stays valid
 *     (phx_solve_stats.recoloured == 0 on the next step).  Dropped pairs leave the touching set, so the next phx_world_contact_events
 *     reports them under end.
 *   - remove and clear touch no manifold: a pair that overlaps is simply new to the next step's UpdatePairs, which gives it a fresh
 *     manifold (the last ones of that step) and joints with zero warm start.
 *   - The other calls: add_body / add_bodies leave the set alone (new bodies are in no pair); remove_bodies / remove_outside drop
 *     every pair that has a removed body and renumber the rest through new[] (increasing on kept bodies: lo < hi and the order both
 *     survive); phx_world_set_state empties the set, as it resets the filters; phx_world_save / load and so a fork carry the set in
 *     HBM beside the blob's layout, as they carry pins; phx_snapshot_export and phx_snapshot_blob_bytes of a snapshot that holds
 *     exclusions return PHX_ERR_STATE (the blob stays layout version 1).  With sleeping enabled add and remove first wake the sleeping
 *     components of the bodies they name, clear those of every pair it removes.  Queries see every body.  Sleeping's edges are manifolds
 *     and units: an excluded pair joined by a pin is still an edge through the pin.
 *   - Sharded worlds carry no exclusions: phx_world_set_shard (shard_count > 1), phx_world_set_comm (a communicator) and
 *     phx_world_reslab return PHX_ERR_STATE while the set is not empty.
 * The host keeps the sorted list; the device a hash table of the keys (lo << 32 | hi, at most half full) and one word per body that
 * says whether the body is in any pair: the sweep row of any other body makes no probe.  O(pairs) bytes cross PCIe when the set or
 * the body numbering changes, nothing per step.  Costs and the data path: DESIGN.md. */
int  phx_world_add_collision_exclusions(phx_world* w, const int32_t* pairs /* 2 per pair */, int32_t count, int32_t* dropped);
int  phx_world_remove_collision_exclusions(phx_world* w, const int32_t* pairs, int32_t count);
int  phx_world_clear_collision_exclusions(phx_world* w);
int  phx_world_get_collision_exclusions(phx_world* w, int32_t* out /* 2 per pair */, int32_t cap /* pairs */, int32_t* count);
/* MATERIALS — per-body friction and restitution.  Every body has a material {friction, restitution}; the default {0.3f, 0.0f} is the
 * reference's kFrictionCoefficient (ref: Solver.cpp:9) and bounce (ref: Solver.cpp:658), and a world whose materials are all the default
 * steps bit for bit as one that never heard of materials.
 *   - Pair values: a contact between bodies a and b uses mu = (a.friction + b.friction) * 0.5f (one rounded sum, an exact halving) and
 *     e = a.restitution > b.restitution ? a.restitution : b.restitution.  Both are exact on equal inputs: default bodies give exactly
 *     0.3f and 0.  The two joints of a body pair share mu and e.
 *   - RefreshJoints (ref: Solver.cpp:664-678): dv = -e * (relV.x * n.x + relV.y * n.y), relV built as the reference builds it from the
 *     solve's body velocities (after IntegrateVelocity): pv1 = ((pos1.y - p1.y) * w1 + v1.x, (p1.x - pos1.x) * w1 + v1.y), the same for
 *     body 2, relV = pv1 - pv2; dst = max(dv - 1, 0); dstVelocity = depth < 1 ? dst - 0.1f : dst.  Source order in both arithmetic forms
 *     (RefreshJoints is never fused).  With e == 0 the result is +0 for every relV, so a joint whose e is 0 skips the velocity gathers.
 *   - Impulse sweep (ref: Solver.cpp:873): the friction limit is accN * mu.  Nothing else changes: PreStep, the displacement sweeps,
 *     the skip tests, the productive thresholds and the static tags stay as they are.
 *   - Valid values: friction finite in [0, 1e6], restitution finite in [0, 1]; anything else is PHX_ERR_INVALID.
 *   - Setting materials: the rules of the edits above.  Between steps only (PHX_ERR_STATE); checked completely before anything is queued
 *     (count >= 0, no NULL array when count > 0, every index in [0, body count), none twice, every value valid; PHX_ERR_INVALID otherwise,
 *     the world unchanged); staged through pinned memory and queued on phx_world_stream(w); before the first step it writes the
 *     host-staged bodies' materials.  A new value applies from the next step's refresh.  It changes no topology: the cached schedule
 *     stays in use (phx_solve_stats.recoloured == 0 on the next step).
 *   - The other calls: add_body / add_bodies give new bodies the default material; remove_bodies / remove_outside move materials with
 *     the kept bodies (through new[]); phx_world_set_state resets every material to the default (a world with materials is checkpointed
 *     as set_state followed by set_materials); the edits, set_inverse_masses, collision filters, queries and contact reports leave them
 *     alone.  The drop-in solver (phx_solver_solve*) keeps the reference's constants.
 *   - Sharded worlds carry no materials: phx_world_set_shard (shard_count > 1), phx_world_set_comm (a communicator) and
 *     phx_world_reslab return PHX_ERR_STATE while some body's material differs from the default.
 *   - The fp16 body-state ablation (phx_solver_set_body_state_bits(phx_world_solver(w), 16)) does not support materials: a step of a
 *     world where some material was ever set (since the last set_state) returns PHX_ERR_STATE.  So does the island trace
 *     (phx_solver_set_trace): such a world's island kernel records none.
 * The solver reads the table only in a world where some material was ever set (since the last set_state); every other world launches
 * the kernels it always did.  Costs and the data path: DESIGN.md. */
typedef struct { float friction, restitution; } phx_material;      /* 8 B; default {0.3f, 0.0f} */
int  phx_world_set_materials(phx_world* w, const int32_t* bodies, const phx_material* materials, int32_t count);
/* every body's material, in index order (cap: room for that many; PHX_ERR_CAPACITY otherwise) */
int  phx_world_get_materials(phx_world* w, phx_material* out, int32_t cap);
/* BODY FLAGS / SENSORS — a body that detects what overlaps it and pushes nothing (a trigger volume).  Every body has a 32-bit flag word,
 * default 0.  One flag is defined, PHX_BODY_SENSOR; any other bit is PHX_ERR_INVALID.  A world whose flags are all 0 steps bit for bit as
 * one that never heard of flags.
 *   - Rule: a manifold is a SENSOR MANIFOLD iff either of its bodies has PHX_BODY_SENSOR.  The change is confined to the Match loop of
 *     RefreshContactJoints (ref: World.cpp:72-149): for every live slot of a sensor manifold, solver_index = -1, and nothing else happens
 *     for that slot — no joint is created and none is re-attached.  Reset and Cleanup are the reference's, unchanged.  So a joint whose
 *     manifold became a sensor manifold is not re-attached and the reference's own swap-remove Cleanup deletes it, in the reference's
 *     order; and a manifold that stops being a sensor manifold gets fresh joints with zero warm-start impulses at the next step, as any
 *     point with solver_index < 0 does.
 *   - Nothing else changes: UpdatePairs, UpdateManifolds, PackManifolds, the narrowphase, the solver and the integrators stay as they
 *     are.  Sensor pairs have manifolds and contact points, so they are in the touching set T(s) of phx_world_contact_events (begin when
 *     something enters the sensor, end when it leaves), phx_world_query_contacts returns their records with PHX_CONTACT_NO_JOINT and
 *     zero impulses, and the markers show them.  A sensor body is otherwise an ordinary body: a dynamic one falls under gravity and is
 *     integrated (nothing holds it up), a static one is a fixed trigger zone.  Queries see sensor bodies like any other body.
 *   - Setting flags: the rules of the edits above.  Between steps only (PHX_ERR_STATE); checked completely before anything is queued
 *     (count >= 0, no NULL array when count > 0, every index in [0, body count), none twice, no unknown bit; PHX_ERR_INVALID otherwise,
 *     the world unchanged); staged through pinned memory and queued on phx_world_stream(w); before the first step it writes the
 *     host-staged bodies' flags.  The call changes only the flag words: the joints go or come at the NEXT step's refresh, and until
 *     that step the getters and the contact reports show the old joints.  The step that deletes or creates joints rebuilds the solver's
 *     schedule as any step that does (phx_solve_stats.recoloured == 1); a flag change that touches no manifold changes no topology.
 *   - The other calls: add_body / add_bodies give new bodies 0; remove_bodies / remove_outside move flags with the kept bodies (through
 *     new[]); phx_world_set_state resets every flag to 0 (a world with sensors is checkpointed as set_state followed by
 *     set_body_flags); the edits, set_inverse_masses, collision filters, materials, queries and contact reports leave them alone.
 *   - Sharded worlds carry no flags: phx_world_set_shard (shard_count > 1), phx_world_set_comm (a communicator) and phx_world_reslab
 *     return PHX_ERR_STATE while some body's flags are not 0.
 * The joint match reads the flags (two 4-byte gathers per manifold) only in a world where some flag was ever set (since the last
 * set_state); every other world launches the kernels it always did.  Costs and the data path: DESIGN.md. */
#define PHX_BODY_SENSOR 1u
int  phx_world_set_body_flags(phx_world* w, const int32_t* bodies, const uint32_t* flags, int32_t count);
/* every body's flags, in index order (cap: room for that many; PHX_ERR_CAPACITY otherwise) */
int  phx_world_get_body_flags(phx_world* w, uint32_t* out, int32_t cap);
/* SHAPES — round bodies.  Every body has a shape {kind, hx, hy}: its kind, PHX_SHAPE_BOX (the default), PHX_SHAPE_CIRCLE or
 * PHX_SHAPE_CAPSULE, and its geom_size.  A box's size is its half extents; a circle's is {r, r}, its radius twice; a capsule's is the half
 * extents of its bounding box in the body's frame, hx > hy > 0: its radius is r = hy and its core segment runs along the body's x axis
 * from pos - xv*a to pos + xv*a with a = hx - hy, one fp32 subtraction, formed the same way wherever it is needed.  A world that never
 * made a circle or a capsule launches exactly the kernels it launched before there were shapes, one whose shape column is active while
 * every body is a box steps bit for bit like it, and one that never made a capsule launches exactly the kernels of a world of boxes and
 * circles: the capsule routines live in instantiations of their own (UpdateManifolds' third, and the queries'), picked by a bit that
 * the first call naming a capsule sets and set_state or a load clears (a load takes the saved world's bit).
 *   - Where it acts: UpdateManifolds (ref: Collider.cpp:211-245).  In front of the separating-axis test the pair's kinds pick the routine;
 *     box/box is the reference's code.  The round routines produce at most one new point per step and hand it to the reference's
 *     MergeCollision (ref: Collider.cpp:58-92) unchanged, so warm starting, isNewlyCreated and the two-slot store work as for boxes (a
 *     pair with a capsule produces up to two, below).  The
 *     normal keeps the stored convention: it points from body2 towards body1, and (p2 - p1) . n >= 0 is the penetration.  Every operation
 *     is fp32 and rounded on its own, sqrtf and / correctly rounded, dot(a, b) = a.x*b.x + a.y*b.y; tests/circle_spec.py states what
 *     follows as the same expressions and the device matches it byte for byte.
 *       circle/circle (r = size.x):  d = pos1 - pos2, l2 = dot(d, d), R = r1 + r2.  No point if l2 > R*R.  l = sqrtf(l2),
 *         n = (d.x / l, d.y / l) if l > 0, else (1, 0).  p1 = pos1 - n*r1, p2 = pos2 + n*r2.
 *       circle C against box B (frame xv, yv, half extents h):  c = C.pos - B.pos, u = dot(c, xv), v = dot(c, yv),
 *         qu = u < -h.x ? -h.x : (u > h.x ? h.x : u), qv likewise.
 *         If qu == u && qv == v (the centre is inside or on the box): pu = h.x - |u|, pv = h.y - |v|; if pu <= pv the face is on x:
 *           N = (u < 0 ? -xv : xv) and qu = (u < 0 ? -h.x : h.x); otherwise on y: N = (v < 0 ? -yv : yv) and qv = (v < 0 ? -h.y : h.y).
 *           N is an exact copy or negation of a stored vector.
 *         Otherwise e = (u - qu, v - qv), l2 = dot(e, e); no point if l2 > r*r; l = sqrtf(l2), N = xv*(e.x / l) + yv*(e.y / l).
 *         Box point = (B.pos + xv*qu) + yv*qv, circle point = C.pos - N*r.  C is body1: n = N, p1 = circle point, p2 = box point;
 *         C is body2: n = -N, p1 = box point, p2 = circle point.
 *     Capsules (tests/capsule_spec.py states what follows as the same expressions; a capsule is the first round shape that rests on a
 *     face, so one point is not enough).  Two building blocks, each yielding a candidate {point on the disc, point on the other shape,
 *     N from the other shape towards the disc, depth}:
 *       disc {c, r} against box B:  the circle/box arithmetic above with the centre c and the radius r; depth = r - l outside, and
 *         r + pu (or r + pv) in the centre-inside branch.
 *       disc {c, rc} against capsule K (frame xv, yv, r = K.size.y, a = K.size.x - K.size.y):  e = c - K.pos, u = dot(e, xv),
 *         v = dot(e, yv), qu = u < -a ? -a : (u > a ? a : u), g = (u - qu, v), l2 = dot(g, g), R = r + rc.  No candidate if l2 > R*R.
 *         l = sqrtf(l2), N = xv*(g.x / l) + yv*(g.y / l) if l > 0, else yv.  Capsule point = (K.pos + xv*qu) + N*r, disc point =
 *         c - N*rc, depth = R - l.  The candidate is unclamped iff qu == u.
 *     The disc's owner is body1: n = N, p1 = disc point, p2 = the other's point; it is body2: n = -N and the points change places.
 *     Candidates per pair, in this order (A = body1 where both are capsules):
 *       capsule / circle:  the circle's disc {pos, size.x} against the capsule.
 *       capsule K / box B: K's end discs {pos - xv*a, r}, {pos + xv*a, r} against B; then B's corners (B.pos + xv*cx) + yv*cy for
 *         (cx, cy) = (-h.x, -h.y), (h.x, -h.y), (-h.x, h.y), (h.x, h.y) as discs of radius 0 against K, each only if unclamped (a
 *         corner nearest an end of the core is the end disc's business).
 *       capsule A / capsule B: A's end discs (radius rA) against B; then B's end discs (radius rB) against A, each only if unclamped
 *         (end against end comes once, from A's side).
 *     Selection: the first point is the candidate of largest depth, the first in order on a tie.  The second is chosen among the
 *     others that are distinct from the first under ContactPoint::Equals(2.0f): sqlen(p1_k - p1_first) > 4.0f AND
 *     sqlen(p2_k - p2_first) > 4.0f; of those the one with the largest sqlen(p1_k - p1_first), the first in order on a tie; none
 *     qualifies: no second point.  First, then second, go through MergeCollision.
 *     What the float64 judge (tests/capsule_reference.py) found and the rule keeps: a second point that comes from an end disc lies on
 *     that disc's circle along the contact normal; where the normal leans by theta from the side's own, that is r*(1 - cos(theta))
 *     inside the capsule's side (second order in the lean, zero at rest on a face); and an end's centre is formed in fp32, so its
 *     normal carries that rounding seen from the distance l.  Known limit: where the core segment itself passes through the other
 *     core (a capsule skewering a box with both ends outside, two crossed segments) the candidates are the nearest end features and
 *     not the minimum translation, and a point may lie on an end disc's circle inside the capsule.  That state is already a tunnelled
 *     one; the rule stays defined and deterministic there.  tests/capsule_corpus.py has the figures.
 *   - Deliberately unchanged: UpdateGeom, IntegratePosition and the broadphase.  A circle's AABB stays the AABB of its frame square
 *     {r, r}: a conservative bound, at most sqrt(2) wider than the disc, so nothing upstream of the narrowphase knows the kind; a
 *     capsule's is that of its frame box {hx, hy}, which contains it and is tight in the body's frame.  The
 *     dead-manifold test (no points and the AABBs apart) and the contact reports stay valid as they are.  The solver sees contact points
 *     and never the shape; pins, links, angles and sliders use body-local anchors.
 *   - Setting shapes: the rules of the edits and of set_materials.  Between steps only (PHX_ERR_STATE); checked completely before
 *     anything is queued (count >= 0, no NULL array when count > 0, every index in [0, body count), none twice, kind in {0, 1, 2}, hx and hy
 *     finite and > 0, hy == hx for a circle, hx > hy for a capsule (hx == hy: use PHX_SHAPE_CIRCLE); PHX_ERR_INVALID otherwise, the
 *     world unchanged); staged through pinned memory and queued on
 *     phx_world_stream(w); before the first step it writes the host-staged records.  The call sets the body's kind and its geom_size
 *     (the record and the resident size) and recomputes the AABB as phx_world_set_poses does (ref: Geom.h:79-85): it is also the edit
 *     that resizes a box.  A sharded or communicator-attached world gets PHX_ERR_STATE.
 *   - Cached state: the call changes no joint topology by itself, so the cached schedule stays valid; cached contact points stay, and
 *     the next step's UpdateManifolds merges or drops them by the ordinary rule; the query index is rebuilt by its next use, as after
 *     set_poses.
 *   - Inverse masses are not touched: the shape is geometry, phx_world_set_inverse_masses is the mass.  AddBody's scale for a box of
 *     half sizes sx, sy is mass = 1e-5f * sx * sy, inertia = mass * (sx*sx + sy*sy) (a quarter of the area, three times the true box
 *     inertia); the circle formula on the same scale is mass = 1e-5f * 0.785398f * r * r, inertia = mass * 1.5f * r * r
 *     (phyx_amd.World.add_circles applies it); the capsule's, with a = hx - hy and r = hy, in this order: mb = 1e-5f*a*r,
 *     mc = 1e-5f*0.785398f*r*r, mass = mb + mc, inertia = mb*(a*a + r*r) + mc*(1.5f*r*r + 3.0f*a*a + 2.546479f*a*r) (the
 *     rectangle's term is the box formula, a -> 0 gives the circle's; phyx_amd.World.add_capsules applies it).
 *   - The other calls: add_body / add_bodies give boxes; remove_bodies / remove_outside move the kind with the kept bodies (through
 *     new[]); phx_world_set_state resets every kind to box (the sizes are in the records; a world with circles or capsules is
 *     checkpointed as set_state followed by set_shapes); phx_world_save / load and so a fork carry the kinds in HBM beside the blob's layout, as they
 *     carry pins; phx_snapshot_export and phx_snapshot_blob_bytes of a snapshot in which a saved kind is not a box return
 *     PHX_ERR_STATE (the blob stays layout version 1).  The edits, set_inverse_masses, filters, materials, flags and contact reports
 *     leave shapes alone.  Queries: QUERIES below.
 *   - Sharded worlds carry no circles or capsules: phx_world_set_shard (shard_count > 1), phx_world_set_comm (a communicator) and phx_world_reslab
 *     return PHX_ERR_STATE while some body is not a box.
 * Every rule above that names circles is written once for "a shape that is not a box" and covers capsules.
 * The kinds are a column of one uint32 per body that exists only once some phx_world_set_shapes call named a circle or a capsule (since
 * the last set_state); a call that names boxes only is the size edit and activates nothing.  Costs and the data path: DESIGN.md. */
#define PHX_SHAPE_BOX    0
#define PHX_SHAPE_CIRCLE 1
#define PHX_SHAPE_CAPSULE 2
typedef struct { int32_t kind; float hx, hy; } phx_shape;   /* 12 B; box: half extents; circle: hx = radius, hy == hx; capsule: the frame box's half extents, hx > hy = radius */
int  phx_world_set_shapes(phx_world* w, const int32_t* bodies, const phx_shape* shapes, int32_t count);
/* every body's {kind, geom_size.x, geom_size.y}, in index order (cap: room for that many; PHX_ERR_CAPACITY otherwise); a world that
 * never set a shape reports boxes */
int  phx_world_get_shapes(phx_world* w, phx_shape* out, int32_t cap);
/* POLYGONS — convex polygon bodies, the fourth kind (PHX_SHAPE_POLYGON).  A polygon is `count` vertices, 3 .. PHX_POLYGON_MAX_VERTICES,
 * in the body's frame (x along xv, y along yv, relative to pos), counter-clockwise; unused slots are stored as +0 and returned as +0.
 * phx_world_set_shapes keeps refusing kind 3 (it names this call); called on a polygon body it turns the body into a box, a circle or a
 * capsule and resets its polygon record to the default (count 0).  phx_world_get_shapes reports kind 3 with the frame box.
 *   - Validity, decided on the host in fp32 (tests/polygon_spec.py poly_valid states the same expressions), all of it before anything is
 *     queued, PHX_ERR_INVALID otherwise and the world unchanged: count in range and every coordinate finite; with e_k = v_(k+1) - v_k
 *     (indices mod count), cross(a, b) = a.x*b.y - a.y*b.x, l_k = sqrtf(dot(e_k, e_k)) and n_k = (e_k.y / l_k, -e_k.x / l_k): every
 *     cross(e_k, e_(k+1)) > 0 (strictly convex, counter-clockwise) and every dot(n_k, v_k) > 0 (the origin strictly inside: it is the
 *     centre of rotation and, by phyx_amd.polygon_inverse_masses, meant to be the centre of mass).  The body-list rules are those of
 *     phx_world_set_shapes: indices in range, none twice, between steps only, PHX_ERR_STATE for a sharded or communicator-attached world.
 *   - What the call sets: the kind; the polygon record {count, v[8], n[8]} with n_k as above, formed by the same fp32 expressions on the
 *     host path (before the first step) and on the device path, so both give the same bytes; the frame box geom_size =
 *     {max |v_k.x|, max |v_k.y|}; the AABB through the unchanged UpdateGeom.  The frame box contains the polygon, so UpdateGeom,
 *     IntegratePosition, the broadphase, the dead-manifold test and the contact reports stay as they are and stay valid.  Staging,
 *     the stream, sleepers, cached points and the query index: as phx_world_set_shapes.
 *   - The records are a column of 132 B per body that exists only once some call named a polygon; a "polygons" bit, set by that call and
 *     cleared by set_state (a load takes the saved world's bit), picks UpdateManifolds' fourth instantiation and the queries' polygon
 *     instantiations.  A world that never made a polygon launches exactly what it launched before.
 *   - The rule (tests/polygon_spec.py is the definition, byte for byte; narrowphase.h restates it).  The box/box, circle and capsule pairs
 *     stay the code they are; a pair with at least one polygon takes the routines below, in which a box is the 4-gon (-hx,-hy), (hx,-hy),
 *     (hx,hy), (-hx,hy) with the exact normals (0,-1), (1,0), (0,1), (-1,0).  World vertex w_k = (pos + xv*v_k.x) + yv*v_k.y, world normal
 *     N_k = xv*n_k.x + yv*n_k.y; every operation fp32, rounded on its own.
 *       polygon / polygon (and polygon / box), A = body1, B = body2:  for each edge i of A, s_i = min_j dot(NA_i, wB_j - wA_i) (the first
 *         j's value, then `<`); sA = the largest s_i, the first on a tie.  No point if sA > 0.  sB likewise, no point if sB > 0.  The
 *         reference face is A's unless sB > sA.  With r0 = wRef_i, r1 = wRef_(i+1), Nr = NRef_i: the incident edge j of the other body
 *         is the one with the smallest dot(Nr, NInc_j), the first on a tie; p0 = wInc_j, p1 = wInc_(j+1).  Clip against the side planes,
 *         with e = r1 - r0:  d0 = dot(p0 - r0, e), d1 = dot(p1 - r0, e); both < 0: no point; d0 < 0: p0 = p0 + (p1 - p0)*(d0 / (d0 - d1));
 *         else d1 < 0: p1 = p1 + (p0 - p1)*(d1 / (d1 - d0)).  Then the same with d0 = dot(r1 - p0, e), d1 = dot(r1 - p1, e).  Each of
 *         p0, p1 in this order with s = dot(Nr, p - r0) <= 0 is a contact: the incident body's point is p, the reference body's
 *         p - Nr*s; the normal is -Nr if the reference is body1, Nr if it is body2.  At most two points, through MergeCollision.
 *       disc {c, r} against polygon P (a candidate as in SHAPES):  g = c - pos, p = (dot(g, xv), dot(g, yv)); s_k = dot(n_k, p - v_k), k
 *         the largest, the first on a tie, s its value.  No candidate if s > r.  If s > 0, with e = v_(k+1) - v_k and t = dot(p - v_k, e):
 *         t < 0 picks the vertex q = v_k, t > dot(e, e) the vertex q = v_(k+1); there h = p - q, l2 = dot(h, h), no candidate if
 *         l2 > r*r, l = sqrtf(l2), N' = (h.x / l, h.y / l), depth = r - l.  Otherwise (s <= 0, or the face region) N' = n_k,
 *         depth = r - s, q = p - n_k*s.  N = xv*N'.x + yv*N'.y, polygon point = (pos + xv*q.x) + yv*q.y, disc point = c - N*r.
 *       circle / polygon:  that one candidate.
 *       capsule K / polygon P:  K's two end discs against P, then P's vertices w_k in index order as discs of radius 0 against K, each
 *         only if unclamped: up to ten candidates, selected by the capsule rule word for word (the deepest first, then the farthest
 *         distinct one under Equals(2.0f), the first in order on ties), as a running selection over the stream of candidates.
 *     Known limit: a deep state in which the face of least penetration is no longer the touching one (a small polygon pushed more than
 *     half way through a thin one): the rule reports the least-penetration face, which is the minimum translation and not the face the
 *     body came in through; the float64 judge (tests/polygon_reference.py) agrees on the depth there and the state is a tunnelled one.
 *   - Queries.  Point p in polygon b iff p is inside b's AABB (closed) AND, with p' the point in the frame (as for a box), every
 *     dot(n_k, p' - v_k) <= 0.  A ray hits polygon b iff b is a candidate and, in the frame (o', d' as in the ray rule), with tin = -inf,
 *     tout = +inf and for k in index order den = dot(n_k, d'), num = dot(n_k, v_k - o'):  den < 0: t = num / den, if t > tin then tin = t
 *     and the entering edge is k;  den > 0: t = num / den, if t < tout then tout = t;  den == 0 and num < 0: a miss.  Then the box rule's
 *     final condition (tin <= tout, tout >= 0, tin <= max_t) and its conventions: t = max(tin, 0), the origin inside gives the normal
 *     (0, 0), otherwise the normal is the entering edge's, xv*n_k.x + yv*n_k.y; ties to the lowest body index.  Oriented-box overlap, box
 *     casts, circle overlap and circle casts see a polygon as its frame box: conservative and mutually consistent, as box queries see
 *     circles and capsules; exact forms are a later change.
 *   - The other calls: add_body / add_bodies give boxes; remove_bodies / remove_outside and spawns carry the column; set_state resets every
 *     kind to box and drops the column; save / load / fork carry it in HBM beside the blob; export of a snapshot with a polygon and
 *     sharding return PHX_ERR_STATE, as for the other kinds that are not boxes.
 * Out of scope: concave or compound bodies, more than 8 vertices, exact polygons in the box and circle overlap and cast queries, polygons
 * in exported blobs and in sharded worlds. */
#define PHX_SHAPE_POLYGON 3
#define PHX_POLYGON_MAX_VERTICES 8
typedef struct { int32_t count; phx_vec2 v[8]; } phx_polygon;   /* 68 B; body-local vertices, counter-clockwise, count in 3 .. 8 */
int  phx_world_set_polygons(phx_world* w, const int32_t* bodies, const phx_polygon* polygons, int32_t count);
/* the polygons of the listed bodies (any order, repeats allowed); a body that is not a polygon gives count 0 and zeros */
int  phx_world_get_polygons(phx_world* w, const int32_t* bodies, phx_polygon* out, int32_t count);
/* QUERIES — where things are: what overlaps a region, what is under a point, what a ray hits first, whether a spot is free for a box
 * or a circle and how far a box or a circle can move before it touches something.  Batched, answered on the device
 * from the resident geometry; nothing of the world crosses PCIe.  Body b's geometry is that of its record (phx_world_get_bodies()[b]):
 * its AABB {aabb_min, aabb_max} and its box {pos, xvector = xv, yvector = yv, geom_size = h (half extents)} (UpdateGeom copies the
 * first three into geom_pos / geom_xvector / geom_yvector, ref: RigidBody.h:38-42).  Every
 * operation below is rounded on its own (the library is built without contraction or fast math): results are exact functions of the
 * records, pinned bit for bit by tests/query_spec.py, which states each formula as the same expression.
 *   - AABB overlap with box q (closed): a.min.x <= q.max.x && a.max.x >= q.min.x && a.min.y <= q.max.y && a.max.y >= q.min.y (as
 *     phx_world_remove_outside tests).  A NaN AABB overlaps nothing.
 *   - Point p in body b iff p is inside b's AABB (closed: a.min.x <= p.x && a.max.x >= p.x && a.min.y <= p.y && a.max.y >= p.y) AND, with
 *     dx = p.x - pos.x, dy = p.y - pos.y:  |dx*xv.x + dy*xv.y| <= h.x  &&  |dx*yv.x + dy*yv.y| <= h.y.  (The fp32 AABB does not exactly
 *     enclose the rounded box test; with the AABB conjunct, pruning by AABBs or tree bounds can never change a result.)
 *   - Ray {ox, oy, dx, dy, max_t}: o + t*d for t in [0, max_t], t in units of d (d need not be unit length).  The slab of one axis with
 *     origin o, direction d and bounds [lo, hi]: if d == 0, all t when lo <= o && o <= hi, else empty (no division by zero); otherwise
 *     a = (lo - o)/d, b = (hi - o)/d, t0 = (a <= b ? a : b), t1 = (a <= b ? b : a).  Over both axes tin = (t0x >= t0y ? t0x : t0y),
 *     tout = (t1x <= t1y ? t1x : t1y), and the test passes iff tin <= tout && tout >= 0 && tin <= max_t.
 *     Body b is a candidate iff its AABB has min <= max on both axes (false for a NaN AABB) and the test passes on the AABB (world
 *     o, d, lo = aabb_min, hi = aabb_max).  The ray hits b iff the test then passes in b's frame: r = o - pos (per component),
 *     o' = (r.x*xv.x + r.y*xv.y, r.x*yv.x + r.y*yv.y), d' = (d.x*xv.x + d.y*xv.y, d.x*yv.x + d.y*yv.y), lo = -h, hi = h.  Then
 *       t      = (tin > 0 ? tin : 0)   (never -0);
 *       normal = (0, 0) if tin < 0 (the origin is inside the box); otherwise the entering axis's stored vector (xv if t0x >= t0y, else
 *                yv), negated when d' on that axis is > 0: always an exact copy or negation of stored floats;
 *       point  = (ox + t*dx, oy + t*dy).
 *     The closest hit is the smallest t, ties to the lowest body index.
 *   - Oriented box {P, X, Y, H} (a position, two frame vectors and half extents, spelled out as in phx_world_set_poses so that nothing is
 *     rounded on the way in; tests/shape_query_spec.py states what follows as the same expressions).  Its extents are
 *       ex = |X.x|*H.x + |Y.x|*H.y,   ey = |X.y|*H.x + |Y.y|*H.y.
 *     Against body b there are four axes, in this order: A0 = X, A1 = Y, A2 = xv, A3 = yv.  With c = P - pos (per component), each
 *     axis A gives, by the same expression for all four (the box's own axes are not special-cased):
 *       s  = c.x*A.x + c.y*A.y
 *       rq = |X.x*A.x + X.y*A.y|*H.x + |Y.x*A.x + Y.y*A.y|*H.y
 *       rb = |xv.x*A.x + xv.y*A.y|*h.x + |yv.x*A.x + yv.y*A.y|*h.y
 *       R  = rq + rb.
 *     The box overlaps b (closed) iff  a.min.x - ex <= P.x && a.max.x + ex >= P.x && a.min.y - ey <= P.y && a.max.y + ey >= P.y  AND
 *     |s| <= R on all four axes.  (Float subtraction and addition are monotone, so a tree node's widened bounds contain its bodies'
 *     widened AABBs: with the AABB conjunct, pruning can never change a result.)  A NaN AABB overlaps nothing.
 *   - Box cast {box, d, max_t}: the box moves as P + t*d for t in [0, max_t].  Per axis, v = d.x*A.x + d.y*A.y and the one-axis slab of
 *     the ray rule is taken with o = s, d = v, lo = -R, hi = R (its d == 0 rule included: no division by zero).  tin is the largest t0
 *     of the four axes and the entering axis the FIRST in order that attains it; tout is the smallest t1.
 *     Body b is a candidate iff its AABB has min <= max on both axes and the ray's two-axis test passes with origin P, direction d,
 *     lo = a.min - (ex, ey), hi = a.max + (ex, ey).  The cast hits b iff b is a candidate, every axis's slab is non-empty and
 *     tin <= tout && tout >= 0 && tin <= max_t.  Then
 *       t      = (tin > 0 ? tin : 0)   (never -0);
 *       normal = (0, 0) if tin < 0 (the boxes overlap at the start); otherwise the entering axis's stored vector (an exact copy of X,
 *                Y, xv or yv), negated when v on that axis is > 0: it points against the motion.
 *     The closest hit is the smallest t, ties to the lowest body index.
 *   - Circles (SHAPES above; r = geom_size.x; tests/circle_spec.py states these as the same expressions).  The AABB query is unchanged: it
 *     uses the record's AABB, that of the frame square.  Point p in circle b iff p is inside b's AABB (closed, as for a box) AND, with
 *     dx = p.x - pos.x, dy = p.y - pos.y:  dx*dx + dy*dy <= r*r.  A ray hits circle b iff b is a candidate (the test on its AABB, as for a
 *     box) and, with rx = ox - pos.x, ry = oy - pos.y, a = dx*dx + dy*dy, b = rx*dx + ry*dy, tc = -b / a (where the line passes the
 *     centre closest), ex = rx + tc*dx, ey = ry + tc*dy (the offset there), h2 = r*r - (ex*ex + ey*ey):
 *     h2 >= 0 (a miss if h2 < 0 or NaN), s = sqrtf(h2 / a), tin = tc - s, tout = tc + s, and tin <= tout && tout >= 0 && tin <= max_t,
 *     the box rule.  Then t = (tin > 0 ? tin : 0), normal = (0, 0) if tin < 0, otherwise ((ex - s*dx) / r, (ey - s*dy) / r), point as
 *     for boxes; ties go to the lowest index, as always.  (The closest-approach form, not the quadratic's discriminant b*b - a*c: that
 *     one squares the origin's distance and loses a small disc's chord a few thousand units away; this one stays within a few
 *     2^-24 * the largest coordinate of the true entry at any distance, tests/query_reference.py.)
 *     Oriented-box queries and box casts see a circle as its frame square {r, r} in the body's frame: both are conservative (they never miss a disc and never report a later t) and consistent with each other, the
 *     two halves of "is this slot free, how far can I drop"; exact discs inside these two are a later change (their bytes are pinned).
 *     A round query shape, exact against boxes and discs alike, is next:
 *   - Capsules (SHAPES above; r = geom_size.y, a = geom_size.x - geom_size.y; tests/capsule_spec.py states these as the same expressions).
 *     Every rule keeps the AABB conjunct the box and the circle have, so pruning can never change a result; the AABB query is
 *     unchanged.  Point p in capsule b iff p is inside b's AABB (closed) AND, with u, v the point in the frame (as for a box) and
 *     qu = (u < -a ? -a : (u > a ? a : u)):  (u-qu)*(u-qu) + v*v <= r*r.  A ray hits capsule b iff b is a candidate and, in the frame
 *     (o', d' as in the ray rule), some part of three passes, tested in this order: 0 the box lo = (-a, -r), hi = (a, r) by the two-axis
 *     slab test; 1 and 2 the discs of radius r at (-a, 0) and (a, 0) by the ray/disc rule with rx = o'.x - centre.x, ry = o'.y and
 *     direction d'.  Each part passes by its own final condition; tin is the smallest passing tin, the first part on a tie; t, point and
 *     the start-inside normal (0, 0) as for the other shapes.  The box part's normal is yv, negated when o'.y + tin*d'.y < 0 (its x
 *     faces are interior: the face is chosen by where the point is, as in the circle cast); a disc part's is the frame normal
 *     (nx / r, ny / r) turned into the world, normal = (xv.x*nx' + yv.x*ny', xv.y*nx' + yv.y*ny').
 *     A query circle {c, r} overlaps capsule b iff the AABB conjunct holds and, with R = r + rb (rb = geom_size.y), u, v of e = c - pos
 *     and qu as above: (u-qu)*(u-qu) + v*v <= R*R.  A circle cast against a capsule body is the ray/capsule rule with origin c and
 *     R = r + rb wherever that rule has the radius, the normals' divisor included.  Oriented-box queries and box casts see a capsule as
 *     its frame box {hx, hy}: conservative, and consistent with each other, exactly as they see a circle as its frame square; their
 *     bytes for worlds without capsules do not move.  (Held to a float64 judge that works by signed distances,
 *     tests/capsule_reference.py.)
 *   - Query circle {c, r} (phx_world_query_circles; tests/round_query_spec.py states what follows as the same expressions): exact
 *     against box bodies and circle bodies alike; rb = geom_size.x of a circle body.  The circle overlaps body b (closed) iff
 *       a.min.x - r <= c.x && a.max.x + r >= c.x && a.min.y - r <= c.y && a.max.y + r >= c.y     (the oriented box's AABB conjunct with
 *     extents (r, r): part of the result, so pruning can never change it; a NaN AABB overlaps nothing)  AND, with e = c - pos (per component),
 *       box body:     u = e.x*xv.x + e.y*xv.y,  v = e.x*yv.x + e.y*yv.y,
 *                     qu = (u < -h.x ? -h.x : (u > h.x ? h.x : u)),  qv = (v < -h.y ? -h.y : (v > h.y ? h.y : v))   (the box's closest point),
 *                     gx = u - qu,  gy = v - qv,  and  gx*gx + gy*gy <= r*r;
 *       circle body:  R = r + rb,  and  e.x*e.x + e.y*e.y <= R*R.
 *   - Circle cast {c, r, d, max_t} (phx_world_cast_circles): the circle moves as c + t*d for t in [0, max_t].  Body b is a candidate iff
 *     its AABB has min <= max on both axes and the ray's two-axis test passes with origin c, direction d, lo = a.min - (r, r),
 *     hi = a.max + (r, r) (the box cast's candidate test with extents (r, r)).  The centre may not enter the body widened by the disc:
 *       circle body:  the ray/disc rule above with origin c and R = r + rb wherever that rule has the radius, the normal's divisor
 *                     included: normal = ((ex - s*dx) / R, (ey - s*dy) / R).
 *       box body:     in the body's frame (o', d' formed as in the ray rule from r = c - pos) the widened box is the union of six convex
 *                     parts, tested in this order: 0 the wide box, lo = (-(h.x + r), -h.y), hi = (h.x + r, h.y); 1 the tall box,
 *                     lo = (-h.x, -(h.y + r)), hi = (h.x, h.y + r); 2 .. 5 the discs of radius r at the corners (-h.x, -h.y),
 *                     (h.x, -h.y), (-h.x, h.y), (h.x, h.y).  A box part is the ray's two-axis slab test on o', d'; a disc part is the
 *                     ray/disc rule with rx = o'.x - corner.x, ry = o'.y - corner.y and direction d'.  A part passes by its rule's own
 *                     final condition, tin <= tout && tout >= 0 && tin <= max_t (and h2 >= 0 for a disc part).  The cast hits b iff
 *                     some part passes; tin is the smallest passing tin, the first part in order on a tie.
 *     Then t = (tin > 0 ? tin : 0) (never -0); normal = (0, 0) if tin < 0 (the circle overlaps b at the start); otherwise the winning
 *     part's: a box part gives the stored vector of the face the centre is on at the entry: with p = (o'.x + tin*d'.x, o'.y + tin*d'.y),
 *     xv if |p.x| - h.x >= |p.y| - h.y, else yv, negated when p on that axis is < 0: an exact copy, as in the ray rule; a disc part gives, with nx = (ex - s*d'.x) / r and ny = (ey - s*d'.y) / r of the ray/disc rule in
 *     the frame, normal = (xv.x*nx + yv.x*ny, xv.y*nx + yv.y*ny).  The closest hit is the smallest t, ties to the lowest body index.
 *     (Held to a float64 judge that works by signed distances, tests/round_query_reference.py.  One part of the rule was changed for
 *     what it found: a box part's normal was first the slab test's entering axis, as in the ray rule, but a cast through the point
 *     where a face of the widened box meets a corner's arc enters the wide or the tall box through its corner, the two axes tie to a
 *     rounding, and the entering axis gave a normal a quarter turn off where the true one is continuous.  The face is now chosen by
 *     where the centre is, which has a margin of r.  DESIGN.md, Queries: circles, has the figures.)
 *   - Nearest body {p, max_dist} (phx_world_query_nearest; tests/near_spec.py is the definition, byte for byte, and states what follows
 *     as the same expressions): how far p is from the nearest body, which body, and where on its surface; exact against all four kinds.
 *     With e = p - pos (per component) and u = e.x*xv.x + e.y*xv.y, v = e.x*yv.x + e.y*yv.y (the point rule's frame coordinates), each
 *     kind gives a signed distance sd (negative inside), an outward normal and a surface point.  "Through the frame" of a frame vector
 *     (lx, ly) is (xv.x*lx + yv.x*ly, xv.y*lx + yv.y*ly); unit(gx, gy, l) is (gx / l, gy / l), and (0, 0) when l == 0.
 *       box:      ax = |u| - h.x, ay = |v| - h.y.  Inside (ax <= 0 && ay <= 0): sd = (ax >= ay ? ax : ay), the face that axis's (x on a
 *                 tie); the normal is the stored xv (yv), negated when u (v) < 0: an exact copy, as in the ray rule; point = p - normal*sd
 *                 (per component).  Outside: qu, qv the clamp of the query circle's rule, gx = u - qu, gy = v - qv,
 *                 sd = sqrtf(gx*gx + gy*gy); gy == 0: the normal is xv negated when u < 0; else gx == 0: yv negated when v < 0 (the face
 *                 regions: exact copies); else (a corner region) unit(gx, gy, sd) through the frame;
 *                 point = ((pos.x + xv.x*qu) + yv.x*qv, (pos.y + xv.y*qu) + yv.y*qv).
 *       circle:   l = sqrtf(e.x*e.x + e.y*e.y), sd = l - r, normal = unit(e.x, e.y, l), point = pos + normal*r (per component; at the
 *                 centre: normal (0, 0), point pos).
 *       capsule:  qu = (u < -a ? -a : (u > a ? a : u)), gx = u - qu, l = sqrtf(gx*gx + v*v), sd = l - r, normal = unit(gx, v, l) through
 *                 the frame, point = ((pos.x + xv.x*qu) + normal.x*r, (pos.y + xv.y*qu) + normal.y*r) (on the core: normal (0, 0) and
 *                 the core's point).
 *       polygon:  the region selection of the disc / polygon rule of POLYGONS: s_k = n_k.x*(u - v_k.x) + n_k.y*(v - v_k.y), k the largest,
 *                 the first on a tie, s its value.  If s > 0, with e' = v_(k+1) - v_k, t = (u - v_k.x)*e'.x + (v - v_k.y)*e'.y: t < 0
 *                 picks the vertex q = v_k, otherwise t > dot(e', e') the vertex q = v_(k+1); there g = (u, v) - q,
 *                 sd = sqrtf(g.x*g.x + g.y*g.y), normal = unit(g.x, g.y, sd) through the frame,
 *                 point = ((pos.x + xv.x*q.x) + yv.x*q.y, (pos.y + xv.y*q.x) + yv.y*q.y).  Otherwise (inside, or a face region): sd = s,
 *                 normal = n_k through the frame, point = p - normal*sd.
 *     The AABB gap of body b: gx = max(max(a.min.x - p.x, p.x - a.max.x), 0), gy likewise, la = sqrtf(gx*gx + gy*gy).  The reported
 *     distance is D = (la > 0 ? (sd >= la ? sd : la) : sd), with -0 reported as +0.  Body b is a candidate iff its AABB has min <= max
 *     on both axes, the query circle's AABB conjunct holds with r = max_dist, and D <= max_dist.  The answer is the candidate with the
 *     smallest D, ties to the lowest body index; distance = D, normal and point the winner's.  max_dist = FLT_MAX means anywhere: a.min - max_dist
 *     and a.max + max_dist saturate or overflow to infinities that keep the conjunct true, and every finite D passes D <= FLT_MAX.  (A point
 *     more than about 1.8e19 from a body squares past the float range on its own: its D is +inf, no candidate under any max_dist.)
 *     (In exact arithmetic sd >= la, the AABB encloses the body; in fp32 sd can fall a rounding short.  With the max in the rule
 *     D >= la holds bit for bit, and la is monotone in the box, so a tree node whose own la is positive and exceeds the best D found
 *     so far holds no body that could win or tie: the walk skips it, and neither that nor the walk's order can change a result.)
 *     Not promised: agreement with phx_world_query_circles at the boundary (gx*gx + gy*gy <= r*r and sqrtf(..) <= r differ by a
 *     rounding, and that call sees a polygon as its frame box).  Inside a body, on its medial set (equal depth to two faces, a circle's
 *     centre, a capsule's core) point and normal jump: the rule's choice there is the one stated.  (Held to a float64 judge,
 *     tests/near_reference.py; DESIGN.md, Queries: nearest, has the figures.)
 * flags: PHX_QUERY_SKIP_STATIC leaves static bodies (inv_mass == 0 && inv_inertia == 0) out of every result (picking without the ground).
 *   A body that sleeps (SLEEPING below) is not static to a query although its inverse masses read 0 while it does: picking a box out of a
 *   resting pile finds it.  A world with sleeping off answers as it always did.
 * Rules:
 *   - Any time, like the gathers: a query sees the geometry at its point of phx_world_stream(w) (between phx_world_pre_solve and
 *     phx_world_finish_step: the geometry before IntegratePosition); the host forms wait for it.
 *   - Host-staged bodies (before the first step, after add_body / set_body_static / set_body_inverse_mass) are uploaded first, as the
 *     removal uploads them.
 *   - The host forms check all their input before anything is queued: count >= 0, no NULL array when count > 0, every value finite,
 *     min <= max for boxes, max_t >= 0 and d != (0, 0) for rays and casts, H > 0 on both axes for oriented boxes, r > 0 for circles, max_dist >= 0 for nearest
 *     queries, flags in {0, PHX_QUERY_SKIP_STATIC}; PHX_ERR_INVALID otherwise.
 *   - The device forms cannot check values: a query with a non-finite component, a ray or cast with max_t < 0 or d == (0, 0), an oriented
 *     box with H.x <= 0 or H.y <= 0, a circle with r <= 0, a nearest query with max_dist < 0 matches nothing.
 *   - An empty world and count == 0 are valid.
 *   - Sharded worlds (replica or slab) answer from their own world, in its local indices; there is no query across ranks.
 *   - A query changes nothing: not the records, the cached solver schedule, the broadphase's state or the next step's result.
 * Two paths give byte-identical results: a scan of the resident arrays (few queries) and a 64-wide tree over the bodies in Morton
 * order (batches), built by the first query after the geometry changed and kept until it changes again.  The library picks one from
 * the kind and number of queries; PHX_QUERY_PATH=scan|index (read when the world is created; any other value makes phx_world_create
 * return PHX_ERR_INVALID) forces one. */
#define PHX_QUERY_SKIP_STATIC 1
typedef struct { int32_t body; float t; phx_vec2 normal, point; } phx_ray_hit;      /* 24 B; no hit: body -1, every other field 0 */
/* boxes: 4 floats per query {min.x, min.y, max.x, max.y}.  offsets: count + 1 entries; the hits of query q are hits[offsets[q] ..
 * offsets[q + 1]), ascending body index; *total = offsets[count].  offsets and *total are filled even when the total exceeds hit_cap:
 * then PHX_ERR_CAPACITY is returned and the contents of hits are unspecified.  A total beyond the int32 range also gives
 * PHX_ERR_CAPACITY (*total is exact; offsets past the int32 range are not). */
int  phx_world_query_aabb(phx_world* w, const float* boxes, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total);
/* points: 2 floats per query; body[q] = the LOWEST index of a body whose box contains the point, -1 if none */
int  phx_world_query_points(phx_world* w, const float* points, int32_t count, int32_t flags, int32_t* body);
/* rays: 5 floats per query {ox, oy, dx, dy, max_t}; out[q] = the closest hit of ray q */
int  phx_world_raycast(phx_world* w, const float* rays, int32_t count, int32_t flags, phx_ray_hit* out);
/* the same two on caller-owned device memory (4-byte aligned), queued on phx_world_stream(w): no host wait, nothing over PCIe */
int  phx_world_query_points_device(phx_world* w, const void* d_points, int32_t count, int32_t flags, void* d_body);
int  phx_world_raycast_device(phx_world* w, const void* d_rays, int32_t count, int32_t flags, void* d_out);
/* boxes: 8 floats per query {pos.x, pos.y, xv.x, xv.y, yv.x, yv.y, h.x, h.y}; the bodies whose box overlaps the query box (closed).
 * Output as phx_world_query_aabb (offsets, ascending hits, *total, PHX_ERR_CAPACITY); no device form: the output size depends on the data. */
int  phx_world_query_boxes(phx_world* w, const float* boxes, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total);
/* casts: 11 floats per query {box[8], dx, dy, max_t}; out[q] = the first body the box touches moving pos + t*d, t in [0, max_t] */
typedef struct { int32_t body; float t; phx_vec2 normal; } phx_shape_hit;      /* 16 B; no hit: body -1, every other field 0 */
int  phx_world_cast_boxes(phx_world* w, const float* casts, int32_t count, int32_t flags, phx_shape_hit* out);
/* the same on caller-owned device memory (4-byte aligned), queued on phx_world_stream(w) */
int  phx_world_cast_boxes_device(phx_world* w, const void* d_casts, int32_t count, int32_t flags, void* d_out);
/* circles: 3 floats per query {c.x, c.y, r}; the bodies whose box or disc overlaps the query circle (closed).  Output as
 * phx_world_query_aabb (offsets, ascending hits, *total, PHX_ERR_CAPACITY); no device form: the output size depends on the data. */
int  phx_world_query_circles(phx_world* w, const float* circles, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total);
/* casts: 6 floats per query {c.x, c.y, r, dx, dy, max_t}; out[q] = the first body the circle touches moving c + t*d, t in [0, max_t] */
int  phx_world_cast_circles(phx_world* w, const float* casts, int32_t count, int32_t flags, phx_shape_hit* out);
/* the same on caller-owned device memory (4-byte aligned), queued on phx_world_stream(w) */
int  phx_world_cast_circles_device(phx_world* w, const void* d_casts, int32_t count, int32_t flags, void* d_out);
/* queries: 3 floats per query {p.x, p.y, max_dist}; out[q] = the body nearest to p within max_dist (max_dist >= 0; FLT_MAX: anywhere),
 * its signed distance (negative: p is inside), the outward normal and the surface point there */
typedef struct { int32_t body; float distance; phx_vec2 normal, point; } phx_near_hit;   /* 24 B; none: body -1, every other field 0 */
int  phx_world_query_nearest(phx_world* w, const float* queries, int32_t count, int32_t flags, phx_near_hit* out);
/* the same on caller-owned device memory (4-byte aligned), queued on phx_world_stream(w); a query with a non-finite component or
 * max_dist < 0 matches nothing */
int  phx_world_query_nearest_device(phx_world* w, const void* d_queries, int32_t count, int32_t flags, void* d_out);
/* CONTACTS — what touches what, and how hard.  Answered on the device from the resident contact cache; nothing of the world crosses
 * PCIe but the answers.  Write s for the state the four getters would return at the call: bodies, manifolds, contact points (cps) and
 * joints.  A manifold m's live slots are k in [0, m.point_count); slot k is contact point cps[m.point_index + k].
 *   - Contacts of body b: one record per live slot k of every manifold m with m.body1 == b or m.body2 == b, cp = cps[m.point_index + k]:
 *       other    = the manifold's other body;   manifold = m's index in phx_world_get_manifolds();   slot = k;
 *       point    = pos_b + delta_b, per component in fp32 (bodies[b].pos plus cp.delta1 if b is body1, cp.delta2 if b is body2; the
 *                  reference's demo draws contact points so, ref: main.cpp:405/411);
 *       normal   = cp.normal if b is body1, its exact negation if b is body2.  The stored normal is the contact axis turned so that
 *                  dot(normal, pos1 - pos2) >= 0 when the point was generated (ref: Collider.cpp GenerateContacts): it points from body2
 *                  towards body1.  So the record's normal points from `other` towards b: the direction the contact pushes b;
 *       normal_impulse, friction_impulse = joints[cp.solver_index]'s accumulated impulses as stored; if solver_index is outside
 *                  [0, joint count) both are 0 and PHX_CONTACT_NO_JOINT is set (set_state does not rule that out, and every
 *                  contact of a sensor pair carries it from the step after the flag was set: BODY FLAGS / SENSORS);
 *       flags    = PHX_CONTACT_NEW if cp.is_newly_created != 0, | PHX_CONTACT_NO_JOINT as above.
 *     Records are ordered by (other, manifold, slot) ascending; the order does not depend on where PackManifolds moved a manifold.
 *     flags PHX_QUERY_SKIP_STATIC leaves out records whose `other` is static (inv_mass == 0 && inv_inertia == 0, as for the queries).
 *     A sleeping `other` is kept, as for the queries.
 *     Output as phx_world_query_aabb: offsets has count + 1 entries, body q's records are out[offsets[q] .. offsets[q + 1]), *total =
 *     offsets[count]; offsets and *total are filled even when the total exceeds cap, which returns PHX_ERR_CAPACITY with the contents of
 *     out unspecified.  A body may be listed more than once: each listing has its own segment.
 *   - Touch events: the touching set T(s) = {(m.body1, m.body2) : m.point_count > 0}, a set of pairs.  The world keeps a baseline B,
 *     empty when the world is created.  phx_world_contact_events returns begin = T(s) \ B and end = B \ T(s), each as {body1, body2}
 *     int32 pairs sorted ascending by (body1, body2), then sets B := T(s).  The semantics are "since the last call": call it once per
 *     step for per-step events; a pair that began and ended between two calls reports nothing.  If either list exceeds its cap, both
 *     totals are still filled, PHX_ERR_CAPACITY is returned and B is NOT advanced (a retry with bigger buffers returns the same events).
 *     What the other calls do to B: a removal remaps it through new[] and drops the pairs with a removed body (new[] is monotonic: B
 *     stays sorted); spawns, edits and set_inverse_masses leave it alone; phx_world_set_state sets B := T(restored state) (a world saved
 *     right after its events call and restored elsewhere reports the same later events); a sharded or communicator-attached world
 *     refuses the events call with PHX_ERR_STATE (a re-slab renumbers bodies).
 *   - Markers (the demo's contact view, ref: main.cpp:393-413): 2 * manifold count records into caller device memory, record i for
 *     contact point i (the slots of manifold i / 2): a live slot has point1 = pos1 + delta1, point2 = pos2 + delta2 (fp32, per
 *     component), live = 1, newly_created = cp.is_newly_created; a dead slot is all zero bytes.  Queued on phx_world_stream(w) with no
 *     host wait; the buffer must be 8-byte aligned; cap (records) < 2 * manifold count gives PHX_ERR_CAPACITY.
 * Rules, the same for all three:
 *   - Between steps only: inside phx_world_pre_solve .. phx_world_finish_step or phx_world_step_begin .. phx_world_step_end they return
 *     PHX_ERR_STATE (the manifolds are mid-update there).
 *   - A pending speculative solve is settled before the joints are read, and host-staged bodies are uploaded first, as for the queries.
 *   - All host input is checked before anything is queued: every body index in [0, body count), count >= 0, no NULL array where one is
 *     needed, caps >= 0, flags in {0, PHX_QUERY_SKIP_STATIC}; PHX_ERR_INVALID otherwise, and nothing changes.
 *   - Contacts and markers of a sharded world answer from the rank's own world, exactly what its getters would return.
 *   - None of them changes the records, the cached schedule, the broadphase or the next step's result; the events call changes B only.
 * Contacts have two paths with byte-identical results: a scan of the manifolds per chunk of listed bodies (few bodies) and a body ->
 * (other, manifold) incidence in CSR form (batches), built by the first call after the contact cache changed and kept until it changes
 * again (a step, a removal, set_state, a change of the body count).  point, normal and the impulses are read at the call.  The library
 * picks a path from the number of listed bodies; PHX_CONTACT_PATH=scan|index (read when the world is created; any other value makes
 * phx_world_create return PHX_ERR_INVALID) forces one. */
#define PHX_CONTACT_NEW 1
#define PHX_CONTACT_NO_JOINT 2
typedef struct {
    int32_t  other, manifold, slot, flags;
    phx_vec2 point, normal;
    float    normal_impulse, friction_impulse;
} phx_contact;                                                                  /* 40 B */
typedef struct { phx_vec2 point1, point2; int32_t live, newly_created; } phx_contact_marker;   /* 24 B */
int  phx_world_query_contacts(phx_world* w, const int32_t* bodies, int32_t count, int32_t flags, int32_t* offsets, phx_contact* out, int32_t cap, int64_t* total);
/* begin / end: 2 int32 per pair; caps in pairs; *begin_total / *end_total: the numbers of pairs */
int  phx_world_contact_events(phx_world* w, int32_t* begin, int32_t begin_cap, int64_t* begin_total, int32_t* end, int32_t end_cap, int64_t* end_total);
int  phx_world_get_contact_markers_device(phx_world* w, void* d_out, int32_t cap);
/* Restore a world from what the four getters above returned (checkpoint / resume; the hand-over of bodies between the ranks of an
 * ownership-sharded world): bodies, the contact cache — manifolds with their two contact-point slots each, ref: Collider.h:57-58 —
 * and the joints with their warm-start impulses (ref: World.h:33).  The broadphase's pair set is rebuilt from the manifolds'
 * body pairs.  A world restored from a saved state steps exactly like the one it was saved from.  Checked: contact_point_count ==
 * 2 * manifold_count, manifold i owns slots 2i and 2i + 1, every joint's bodies are its manifold's and its contact point's
 * solver_index points back at it; PHX_ERR_INVALID otherwise.  Any number of bodies (the world's previous content is dropped). */
int  phx_world_set_state(phx_world* w, const phx_rigid_body* bodies, int32_t body_count, const phx_manifold* manifolds, int32_t manifold_count,
                         const phx_contact_point* contact_points, int32_t contact_point_count, const phx_contact_joint* joints, int32_t joint_count);
/* SNAPSHOTS — save a whole world, try something, put it back (rollback, "try N actions from the same state", an environment reset, a saved
 * game), without the state leaving HBM.  A phx_snapshot owns device memory on its device; it grows geometrically and every save reuses it.
 *   - What a snapshot holds: the complete state World::Update carries from step to step, plus the per-body columns:
 *       the bodies' 128-byte records as phx_world_get_bodies would return them at the save (a record the steps have left stale is brought up
 *       to date from the resident arrays on the way; pending accelerations ride in the records, as they do through phx_world_set_state);
 *       the manifolds, their contact-point slots, the joints with their warm-start impulses;
 *       the three optional columns (collision filters, materials, body flags), each with its "ever set" bit (and, beside the blob's
 *       layout, the shapes' kinds: SHAPES above);
 *       the touch events' baseline B AS IT IS (not T(state): the next phx_world_contact_events after a load reports what it would have
 *       reported had the save and the load never happened).
 *   - What it does NOT hold, and a load leaves alone: gravity, the shard and the communicator, phase timing, the paths chosen from the
 *     environment (PHX_QUERY_PATH, PHX_CONTACT_PATH, ...), the fp16 body-state ablation and every other setting of the world's solver.
 *     A snapshot forked into a fresh world needs its gravity set by the caller, and its pin iteration count (phx_world_set_pin_iterations)
 *     if it is not the default: the pins and their impulses are saved, the number of sweeps is a setting of the world and is not.
 *   - Definition of load: after phx_world_load(w, s) the world is exactly what these calls would have made of it, byte for byte in every
 *     getter and in every later step:
 *       1. phx_world_set_state of the four saved arrays;
 *       2. phx_world_set_collision_filters of the saved filters, if that column was active in s;
 *       3. phx_world_set_materials of the saved materials, if that column was active in s;
 *       4. phx_world_set_body_flags of the saved flags, if that column was active in s;
 *       5. B := the saved B.
 *     A column that was inactive in s is the default for every body afterwards.  Everything set_state resets is reset: the broadphase's
 *     pair set becomes the saved manifolds' pairs, the query and contact indexes are rebuilt by their next use, and the cached solver
 *     schedule is rebuilt at the next step (phx_solve_stats.recoloured != 0).  s is unchanged and can be loaded again, into any world on
 *     its device (a FORK: world A saves, world B loads).
 *   - Rules, those of the edits, the removal and the spawn: between steps only (PHX_ERR_STATE inside pre_solve .. finish_step or
 *     step_begin .. step_end); a sharded or communicator-attached world gets PHX_ERR_STATE from both calls; a snapshot that was never
 *     filled gives PHX_ERR_STATE from load, counts, blob_bytes and export; a snapshot of another device gives PHX_ERR_INVALID; a NULL
 *     handle gives PHX_ERR_INVALID.  Host-staged bodies (before the first step, after add_body / set_body_static /
 *     set_body_inverse_mass) are uploaded before a save, as the removal uploads them; a load drops them with the rest of the old world.
 *     A save into a filled snapshot overwrites it.  A call that fails leaves the world's and the snapshot's contents as they were.
 *   - Where the host waits: nowhere new.  Both calls are queued on phx_world_stream(w): one kernel each (and, for a load, the reset of
 *     the pair set).  They wait only to settle an unverified solve, as the removal does, and where a buffer has to grow or the pair
 *     set's table is replaced.  The counts are on the host between steps, so nothing is read back and nothing of the state crosses PCIe.
 *     Between worlds: a save records an event that a later load's stream waits for, a load records one that the next save into s, export,
 *     import and destroy wait for — no host wait, no extra stream.
 *   - The blob: the one form that leaves the device (disk, another machine, another device).  phx_snapshot_export writes it, phx_snapshot_import
 *     checks it completely before anything is allocated or copied and fills the snapshot from it.  Little-endian; every section starts at a
 *     multiple of 16 bytes from the start of the blob and the bytes between sections are zero:
 *          0  char[8]   "PHXSNAP\0"                  8  uint32  layout version (1)         12  uint32  header bytes (128)
 *         16  int32     bodies n                     20  int32   manifolds m                24  int32   contact points (2 m)
 *         28  int32     joints j                     32  uint32  column bits: 1 filters, 2 materials, 4 flags (clear: all default, no section)
 *         36  int32     baseline pairs t             40  uint64  total bytes                48  uint64[8] section offsets     112  16 zero bytes
 *       sections, in this order, the first at 128, each next one at the end of the one before rounded up to 16, the total the last end
 *       rounded up to 16:  bodies n x 128 (phx_rigid_body) | manifolds m x 16 | contact points 2m x 32 | joints j x 20 |
 *       filters n x 16 ({category, mask, group, 0}: the device's own granule) | materials n x 8 | flags n x 4 |
 *       baseline t x 8 (uint64 (body1 << 32) | body2, strictly increasing).
 *       Column bit 8 (CONTINUOUS BODIES) adds a ninth section behind the baseline, n x 16 {rc, start.x, start.y, 0}, whose offset is the
 *       uint64 at byte 112 (bytes 120 .. 127 stay zero); without the bit bytes 112 .. 127 are zero and nothing else changes.
 *     The device side of a snapshot has this layout too: export and import are one copy each.  phx_snapshot_blob_check is the single
 *     validator (host only): the header, every size and offset against `bytes` in 64-bit arithmetic that cannot overflow, everything
 *     phx_world_set_state checks, the ranges the setters enforce (friction finite in [0, 1e6], restitution in [0, 1], no unknown flag bit,
 *     a filter's fourth word zero, zero bytes between the sections) and the baseline strictly increasing with indices in range; PHX_ERR_INVALID with a message
 *     (phx_last_error) that names the first violated rule.  phx_snapshot_blob_pack makes a blob from host arrays — what the getters
 *     return — so a state from elsewhere can become a snapshot: a NULL column means every body has the default, a NULL baseline means
 *     T(state), as phx_world_set_state makes it; baseline_pairs are {body1, body2} int32 pairs.  *bytes always receives the size;
 *     PHX_ERR_CAPACITY when cap is smaller (blob may then be NULL).
 * Costs and the data path: DESIGN.md. */
typedef struct phx_snapshot phx_snapshot;
int  phx_snapshot_create(phx_snapshot** out, int device);      /* empty; owns device memory, grows geometrically, reused by every save */
void phx_snapshot_destroy(phx_snapshot* s);
int  phx_world_save(phx_world* w, phx_snapshot* s);             /* s := the world */
int  phx_world_load(phx_world* w, phx_snapshot* s);             /* the world := s (s unchanged; any world on s's device) */
int  phx_snapshot_counts(phx_snapshot* s, int32_t* bodies, int32_t* manifolds, int32_t* contact_points, int32_t* joints);
int  phx_snapshot_blob_bytes(phx_snapshot* s, size_t* bytes);
int  phx_snapshot_export(phx_snapshot* s, void* blob, size_t cap);          /* device -> one host blob */
int  phx_snapshot_import(phx_snapshot* s, const void* blob, size_t bytes);  /* checked completely first */
/* host only, no device needed */
int  phx_snapshot_blob_check(const void* blob, size_t bytes);
int  phx_snapshot_blob_pack(const phx_rigid_body* bodies, int32_t body_count, const phx_manifold* manifolds, int32_t manifold_count,
                            const phx_contact_point* cps, int32_t cp_count, const phx_contact_joint* joints, int32_t joint_count,
                            const phx_collision_filter* filters, const phx_material* materials, const uint32_t* flags,
                            const int32_t* baseline_pairs, int32_t baseline_count,
                            void* blob, size_t cap, size_t* bytes);

/* PINS — hold a point of one body on a point of another (a revolute joint), or on a fixed point of the world (body2 = -1): chains,
 * pendulums, hinges, a dragged body that follows the cursor rigidly.  The reference has no such constraint; tests/pin_spec.py is the
 * definition (scalar float32, every operation rounded on its own, no fused multiply-add in either phx_arith_mode, IEEE division) and
 * the device matches it byte for byte.
 *   - anchor1 / anchor2 are in the bodies' own frames: the world point of an anchor is pos + xVector * a.x + yVector * a.y.  With
 *     body2 == -1, anchor2 is a world point.  impulse is the accumulated impulse: the warm start, carried from step to step, 0 for a new
 *     pin unless the caller restores one.
 *   - The pass runs once per step at the end of phx_world_pre_solve: IntegrateVelocity and RefreshContactJoints are done, SolveJoints
 *     has not started.  It reads positions and frames as the last IntegratePosition left them and reads and writes velocity and
 *     angularVelocity only; contacts are solved afterwards on the velocities the pins left, so a contact has the last word.  Per pin,
 *     with m, i the inverse mass and inertia (0 for the world), ra, rb the rotated anchors (rb = 0 for the world), and w x r = (w r.y, -w r.x):
 *     the reference's angularVelocity is clockwise-positive (IntegratePosition rotates by -w dt, ref: World.cpp:63; the contact limiters
 *     project it with n x r, ref: Solver.cpp:559), so that is the velocity its w gives the point r, and P at r changes w by -i (r x P):
 *         C    = (posB + rb) - (posA + ra)                      (world pin: anchor2 - (posA + ra))
 *         k11  = mA + mB + iA ra.y^2 + iB rb.y^2,  k12 = -iA ra.x ra.y - iB rb.x rb.y,  k22 = mA + mB + iA ra.x^2 + iB rb.x^2
 *         det  = k11 k22 - k12^2;  a pin with !(det > 2^-20 (k11 k22)) is INACTIVE this step: impulse := 0, nothing else (the floor is
 *                the float32 det expression's rounding noise, at most 14 x 2^-24 k11 k22: a singular K - invMass 0, invInertia > 0, pinned off-centre - is not solved with 1/noise)
 *         bias = C * (0.2f / dt);  warm start: apply impulse;  n sweeps: cdot = (vB + wB x rb) - (vA + wA x ra), rhs = -(cdot + bias),
 *         d = (1/det) * (k22 rhs.x - k12 rhs.y, k11 rhs.y - k12 rhs.x), impulse += d, apply d
 *         apply P: vA -= mA P, wA += iA (ra.x P.y - ra.y P.x), vB += mB P, wB -= iB (rb.x P.y - rb.y P.x)   (a static body is not written)
 *     n = phx_world_set_pin_iterations (1 .. 64, default 8), a setting of the world like gravity.  There is no cap on the bias: a pin
 *     whose anchor is moved far in one step pulls hard.  The bias is part of the accumulated impulse, hence of the next step's warm start:
 *     a chain whose tension the n sweeps do not carry from end to end within a step oscillates, and the oscillation grows (the spec's
 *     hanging chain of 16 links diverges at n = 8 and rests at n = 32: tests/pin_spec.py) - give long chains more sweeps.  Pins do not stop their two bodies from colliding: collision exclusions (COLLISION EXCLUSIONS) or filters do that.
 *   - Order is semantics: prestep and warm start in the slot order of the pin schedule, then n sweeps in slot order.  The schedule
 *     (phx_world_get_pin_schedule, host-only twin phx_pin_schedule) is phx_schedule_groups' with one pin per unit, the world anchor as one
 *     virtual static body (index body_count) and at most `group_pins` pins per group (256; PHX_PIN_GROUP_PINS=n, 1 .. 256, read when a
 *     world is created, lowers it for tests): connected components binned into groups that one workgroup solves out of LDS in ONE launch,
 *     whatever does not fit in one trailing group swept class by class out of HBM.  It is rebuilt on the host, lazily at the next step,
 *     when the pin set or the static set changed (add_pins, remove_pins, a removal of bodies that took pins with it, set_inverse_masses,
 *     set_body_static, set_body_inverse_mass, set_state, load); anchor edits, spawns and every other call keep it.  O(pins) bytes cross PCIe at such
 *     a change, nothing per step.  phx_world_pin_schedule_builds counts the builds.
 *   - Rules, those of the edits: between steps only (PHX_ERR_STATE otherwise); arguments are checked completely before anything is queued
 *     and a failed check (PHX_ERR_INVALID) leaves the world unchanged: count >= 0, no NULL array when count > 0, body1 in range, body2 in
 *     range or -1, body1 != body2, anchors and impulse finite, pin indices in range and distinct.  An empty call is a true no-op.  A pin
 *     between two static bodies is accepted and merely inactive.  remove_pins keeps the others' order (indices shift).  Before the first
 *     step the pins wait on the host with the host-staged bodies.
 *   - The other calls: phx_world_remove_bodies / remove_outside drop every pin that has a removed body, remap the rest through new[] and
 *     keep their order; phx_world_set_state drops every pin; phx_world_save / load carry the pins with their impulses in HBM (the
 *     definition of load gains: 6. phx_world_add_pins of the saved pins), but the blob stays layout version 1 and holds none, so
 *     phx_snapshot_export and phx_snapshot_blob_bytes of a snapshot that holds pins return PHX_ERR_STATE; sharded worlds carry none:
 *     phx_world_set_shard (count > 1), set_comm and reslab return PHX_ERR_STATE while a pin exists, and so does add_pins on a sharded world.
 *     A world without pins launches nothing new and allocates nothing new. */
typedef struct { int32_t body1, body2; phx_vec2 anchor1, anchor2; phx_vec2 impulse; } phx_pin;   /* 32 B */
int  phx_world_add_pins(phx_world* w, const phx_pin* pins, int32_t count, int32_t* first);      /* *first (may be NULL) = index of the first new pin */
int  phx_world_remove_pins(phx_world* w, const int32_t* pins, int32_t count);
int  phx_world_set_pin_anchors(phx_world* w, const int32_t* pins, const float* anchors /* 4 per pin: anchor1, anchor2 */, int32_t count);
int  phx_world_get_pins(phx_world* w, phx_pin* out, int32_t cap);
int  phx_world_pin_count(phx_world* w, int32_t* count);
int  phx_world_set_pin_iterations(phx_world* w, int32_t n);
int  phx_world_get_pin_iterations(phx_world* w, int32_t* n);
int  phx_world_pin_schedule_builds(phx_world* w, int64_t* builds);
/* The schedule the next step's pin pass uses (built now unless current; between steps only): order[k] = the pin in slot k, class c owns
 * slots [class_offsets[c], class_offsets[c + 1]), group g owns slots [group_offsets[g], group_offsets[g + 1]); the first *lds_group_count
 * groups run one workgroup each out of LDS, the rest (at most one) out of HBM.  Pass NULL arrays (cap 0) to ask for the counts.
 * With links (LINKS) the slots hold units - pins, then links - and order needs room for pin_count + link_count of them. */
int  phx_world_get_pin_schedule(phx_world* w, int32_t* order, int32_t order_cap, int32_t* class_offsets, int32_t class_cap, int32_t* class_count,
                                int32_t* group_offsets, int32_t group_cap, int32_t* group_count, int32_t* lds_group_count);
/* host only, no device needed: the same schedule from the pins' bodies (body2 = -1: the world) and the bodies' static flags */
int  phx_pin_schedule(const int32_t* body1, const int32_t* body2, int32_t pin_count, const uint8_t* is_static, int32_t body_count, int32_t group_pins,
                      int32_t* order, int32_t* class_offsets, int32_t class_cap, int32_t* class_count,
                      int32_t* group_offsets, int32_t group_cap, int32_t* group_count, int32_t* lds_group_count);

/* LINKS — constrain the DISTANCE between a point of one body and a point of another, or of the world (body2 = -1): a rigid rod, a rope
 * that is slack until it is taut, a spring (a soft drag where a pin pulls hard).  tests/link_spec.py is the definition (scalar float32,
 * every operation rounded on its own, no fused multiply-add, IEEE division, correctly rounded square root) and the device matches it byte
 * for byte.  Links are solved IN the pin pass: its units are the pins followed by the links (unit u < pin_count is pin u, otherwise link
 * u - pin_count), one schedule, one launch, one Gauss-Seidel sweep in which a rope tied to a chain link interleaves with the chain's pins.
 * Wherever PINS says "pin" of the schedule it means a unit: PHX_PIN_GROUP_PINS caps units per group, phx_world_set_pin_iterations is the
 * pass's sweep count, phx_world_get_pin_schedule returns units (order_cap >= pin_count + link_count), phx_world_pin_schedule_builds
 * counts the builds of the one schedule, which add_links / remove_links rebuild in addition to PINS' causes.
 *   - Anchors and bodies as for a pin.  impulse is the accumulated scalar impulse along the axis: the warm start, 0 for a new link.
 *     With ra, rb the rotated anchors exactly as the pin's:
 *         d = (posB + rb) - (posA + ra),  len = sqrt(d.x d.x + d.y d.y),  n = d / len,  kinv = mA + mB + iA (ra x n)^2 + iB (rb x n)^2
 *     A link with !(len > 2^-10) or !(kinv > 0) is INACTIVE this step: impulse := 0, nothing else (below 2^-10 the axis is the rounding
 *     noise of the position subtraction; kinv <= 0: both ends static or the world).
 *   - The kind follows from the data:
 *         rod     min_length == max_length == L, hertz == 0: C = len - L, impulse unbounded, bias = C (0.2f / dt), gamma = 0
 *         spring  min_length == max_length == L, hertz > 0 (the Box2D soft constraint): mass = 1 / kinv, w = 6.2831855f hertz,
 *                 dmp = 2 mass damping_ratio w, k = mass w^2, gamma = 1 / (dt (dmp + dt k)), bias = C dt k gamma, kinv += gamma
 *         rope / limits  min_length < max_length, hertz == 0: the engaged limit is decided at the prestep - len >= max: C = len - max,
 *                 impulse <= 0; len <= min: C = len - min, impulse >= 0; otherwise the link is IDLE this step: impulse := 0, nothing
 *                 else.  A rope is min_length = 0.  This is deliberately NOT speculative: a limit engages the step after the length
 *                 overshoots it, and the bias (that of the rod) pulls it back; until then the bodies move exactly as without the link.
 *     warm start: impulse clamped to the engaged limit's range, P = impulse n applied with the pin's apply;  n sweeps:
 *         cdot = n . ((vB + wB x rb) - (vA + wA x ra)),  d = -(1 / kinv) ((cdot + bias) + gamma impulse)
 *         rod, spring: impulse += d, apply d n;  limits: new = clamp(impulse + d) (x < lo ? lo : x > hi ? hi : x, so a NaN passes),
 *         apply (new - impulse) n, impulse = new
 *   - The calls follow the pins' rules word for word (between steps, checked completely first, PHX_ERR_INVALID leaves the world
 *     unchanged, an empty call is a no-op, before the first step the links wait on the host).  Checked: the pins' body rules, every float
 *     finite, 0 <= min_length <= max_length, hertz >= 0, damping_ratio >= 0, hertz > 0 only with min_length == max_length, reserved == 0;
 *     set_link_lengths is checked against the link's stored hertz.  set_link_anchors and set_link_lengths keep the schedule.
 *   - The other calls, as for pins: remove_bodies / remove_outside drop the links of removed bodies and remap the rest; set_state drops
 *     every link; save / load carry the links with their impulses in HBM; phx_snapshot_export and phx_snapshot_blob_bytes of a snapshot
 *     that holds links return PHX_ERR_STATE (the blob stays layout version 1); set_shard (count > 1), set_comm, reslab and add_links on a
 *     sharded world return PHX_ERR_STATE.  A world without links allocates and launches exactly what it did without them. */
typedef struct { int32_t body1, body2; phx_vec2 anchor1, anchor2; float min_length, max_length; float hertz, damping_ratio;
                 float impulse; uint32_t reserved; } phx_link;   /* 48 B */
int  phx_world_add_links(phx_world* w, const phx_link* links, int32_t count, int32_t* first);   /* *first (may be NULL) = index of the first new link */
int  phx_world_remove_links(phx_world* w, const int32_t* links, int32_t count);
int  phx_world_set_link_anchors(phx_world* w, const int32_t* links, const float* anchors /* 4 per link: anchor1, anchor2 */, int32_t count);
int  phx_world_set_link_lengths(phx_world* w, const int32_t* links, const float* lengths /* 2 per link: min, max */, int32_t count);
int  phx_world_get_links(phx_world* w, phx_link* out, int32_t cap);
int  phx_world_link_count(phx_world* w, int32_t* count);

/* ANGLES — constrain the relative ANGLE of two bodies, or of a body against the world (body2 = -1: the identity frame, w = 0): a lock
 * (with a pin: a weld), limits (a door's stops, an elbow), a torsion spring, a motor (a driven or braked wheel).  tests/angle_spec.py is
 * the definition (scalar float32, every operation rounded on its own, no fused multiply-add, IEEE division) and the device matches it
 * byte for byte.  Angles are the pin pass's third kind of unit: the units are the pins, then the links, then the angles (unit
 * u < pin_count is pin u, u < pin_count + link_count is link u - pin_count, any other is angle u - pin_count - link_count), one
 * schedule, one launch, one Gauss-Seidel sweep.  Wherever PINS and LINKS say "pin" or "unit" of the schedule the angles count too:
 * phx_world_get_pin_schedule needs order_cap >= pin_count + link_count + angle_count, add_angles / remove_angles rebuild the schedule.
 *   - The angle.  With xA, xB the bodies' xVector (the world: (1, 0)):
 *         c = xA.x xB.x + xA.y xB.y,  s = xA.x xB.y - xA.y xB.x,  theta = (float)atan2((double)(-s), (double)c)
 *     in the prestep only (the double-precision atan2 rounded to float, as IntegratePosition's cos / sin).  angularVelocity is
 *     clockwise-positive (PINS), theta is the clockwise angle of B against A and d theta / dt = wB - wA.  Against the world the world is
 *     B: a body1 that turns with w > 0 LOSES w dt of theta per step (put the reference body first to read it the other way).
 *         mid = (lower + upper) 0.5f,  half = (upper - lower) 0.5f,  phi = theta - mid, wrapped once: phi > PI: phi - TWO_PI,
 *         phi < -PI: phi + TWO_PI, with PI = 3.1415927f, TWO_PI = 6.2831855f
 *     so a lock at 3 rad does not jump where theta crosses pi, and a range wider than 2 PI is never engaged (a pure motor).
 *   - kinv = iA + iB.  An angle with !(kinv > 0) is INACTIVE this step: impulse := 0, motor_impulse := 0, nothing else.
 *   - The row L follows from the data (decided at the prestep, not speculative, as a rope's limit):
 *         lock    lower == upper, hertz == 0: C = phi, impulse unbounded, bias = C (0.2f / dt), gamma = 0
 *         spring  lower == upper, hertz > 0 (the Box2D soft constraint): C = phi, mass = 1 / kinv, w = 6.2831855f hertz,
 *                 dmp = 2 mass damping_ratio w, k = mass w^2, gamma = 1 / (dt (dmp + dt k)), bias = C dt k gamma
 *         limits  lower < upper: phi >= half: C = phi - half, impulse <= 0; phi <= -half: C = phi + half, impulse >= 0 (bias as the
 *                 lock's); otherwise L is IDLE this step: impulse := 0
 *     The row M, the motor, is on where max_torque > 0: it drives wB - wA to motor_speed, its accumulated motor_impulse clamped to
 *     +- max_torque dt.  Off: motor_impulse := 0.  An angle with neither row engaged writes both impulses 0 and nothing else: its bodies
 *     move bit for bit as without it.
 *   - warm start: motor_impulse clamped to its range, then impulse clamped to the engaged limit's, each applied where its row is on, M
 *     first.  n sweeps, M first, then L (Box2D's order), each on the velocities the other left:
 *         M: cdot = wB - wA, d = -((1 / kinv) (cdot - motor_speed)), new = clamp(motor_impulse + d), apply new - motor_impulse
 *         L: cdot = wB - wA, d = -((1 / (kinv + gamma)) ((cdot + bias) + gamma impulse)); lock, spring: impulse += d, apply d;
 *            limits: new = clamp(impulse + d), apply new - impulse          (clamp: x < lo ? lo : x > hi ? hi : x, so a NaN passes)
 *         apply d: wA -= iA d, wB += iB d.  Linear velocities are not touched; a static body is not written.
 *   - The calls follow the pins' and links' rules word for word.  Checked at add: the pins' body rules, every float finite,
 *     lower <= upper, hertz >= 0, damping_ratio >= 0, max_torque >= 0, hertz > 0 only with lower == upper.  set_angle_limits is checked
 *     against the angle's stored hertz, set_angle_motors wants finite values and max_torque >= 0; both keep the schedule.  There are no
 *     anchors to set.
 *   - The other calls, as for links: remove_bodies / remove_outside drop the angles of removed bodies and remap the rest; set_state drops
 *     every angle; save / load carry the angles with both impulses in HBM; phx_snapshot_export and phx_snapshot_blob_bytes of a snapshot
 *     that holds angles return PHX_ERR_STATE; set_shard (count > 1), set_comm, reslab and add_angles on a sharded world return
 *     PHX_ERR_STATE.  A world without angles allocates and launches exactly what it did without them. */
typedef struct { int32_t body1, body2;            /* body2 = -1: the world (identity frame, w = 0) */
                 float lower, upper;               /* radians, on the relative angle theta */
                 float hertz, damping_ratio;       /* > 0 only with lower == upper: a torsion spring */
                 float motor_speed, max_torque;    /* max_torque > 0: the motor row is on */
                 float impulse, motor_impulse;     /* accumulated angular impulses: the warm start */
} phx_angle;                                       /* 40 B */
int  phx_world_add_angles(phx_world* w, const phx_angle* angles, int32_t count, int32_t* first);   /* *first (may be NULL) = index of the first new angle */
int  phx_world_remove_angles(phx_world* w, const int32_t* angles, int32_t count);
int  phx_world_set_angle_limits(phx_world* w, const int32_t* angles, const float* limits /* 2 per angle: lower, upper */, int32_t count);
int  phx_world_set_angle_motors(phx_world* w, const int32_t* angles, const float* motors /* 2 per angle: motor_speed, max_torque */, int32_t count);
int  phx_world_get_angles(phx_world* w, phx_angle* out, int32_t cap);
int  phx_world_angle_count(phx_world* w, int32_t* count);

/* SLIDERS — hold a point of body1 (the carriage) ON A LINE of body2 (the rail; body2 = -1: the world): a piston, an elevator, a sliding
 * door, with an angle lock a prismatic joint, without one a wheel's suspension.  tests/slider_spec.py is the definition (scalar float32,
 * every operation rounded on its own, no fused multiply-add, IEEE division, correctly rounded sqrt) and the device matches it byte for
 * byte.  Sliders are the pin pass's fourth kind of unit, behind the angles: unit u >= pin_count + link_count + angle_count is slider
 * u - pin_count - link_count - angle_count; one schedule, one launch, one Gauss-Seidel sweep.  Wherever PINS, LINKS and ANGLES say "pin"
 * or "unit" of the schedule the sliders count too: phx_world_get_pin_schedule needs order_cap >= pin_count + link_count + angle_count +
 * slider_count, add_sliders / remove_sliders rebuild the schedule.
 *   - The geometry, in the prestep.  ra, rb: the rotated anchors, as a pin's.  e = (posA + ra) - (posB + rb) (the world: - anchor2).
 *     a = the axis rotated by body2's frame as an anchor is (the world: the axis itself), len = sqrtf(a.x a.x + a.y a.y), n = a / len,
 *     t = (-n.y, n.x).  s = n . e is the carriage's coordinate along the rail, t . e its distance off it.
 *   - Both rows act at the carriage's anchor point on both bodies: A's arm is ra, B's is rb' = rb + e (which carries the wB term of an
 *     axis that turns with the rail).  With w x r = (w r.y, -w r.x) (angularVelocity is clockwise-positive, PINS) and
 *     r x u = r.x u.y - r.y u.x, for u in {t, n}:
 *         cdot_u = u . ((vA + wA x ra) - (vB + wB x rb'))
 *         kinv_u = ((mA + mB) + (iA (ra x u)) (ra x u)) + (iB (rb' x u)) (rb' x u)
 *         apply P = lambda u:  vA += mA P,  wA -= iA (ra x P),  vB -= mB P,  wB += iB (rb' x P)       (a static body is not written)
 *     A carriage that moves along +n gains s.
 *   - !(kinv_t > 0): the slider is INACTIVE this step: its three impulses := 0, nothing else.  !(kinv_n > 0) with kinv_t > 0: rows L and
 *     M are off, axis_impulse := 0, motor_impulse := 0, and P runs.  Nothing divides by |e|: e = 0 is an ordinary case.
 *   - The rows:
 *         P  perpendicular: C = t . e, impulse unbounded, bias = C (0.2f / dt); on whenever the slider is active
 *         L  along the axis, on s, ANGLES' row L word for word: lower == upper, hertz == 0 a lock (C = s - lower); lower == upper,
 *            hertz > 0 a spring towards s = lower (the links' soft constraint with mass = 1 / kinv_n); lower < upper limits:
 *            s >= upper: C = s - upper, impulse <= 0; s <= lower: C = s - lower, impulse >= 0; otherwise IDLE this step:
 *            axis_impulse := 0.  Decided at the prestep, not speculative, as a rope's limit.
 *         M  the motor, on where max_force > 0: it drives cdot_n to motor_speed, its accumulated motor_impulse clamped to
 *            +- max_force dt.  Off: motor_impulse := 0.
 *   - warm start: motor_impulse and axis_impulse clamped to their ranges, then M, L, P applied, each where its row is on.  n sweeps of
 *     M, then L, then P, each on the velocities the row before left: the hard row has the last word.
 *         M: d = -((1 / kinv_n) (cdot_n - motor_speed)), new = clamp(motor_impulse + d), apply new - motor_impulse along n
 *         L: d = -((1 / (kinv_n + gamma)) ((cdot_n + bias) + gamma axis_impulse)); lock, spring: axis_impulse += d; limits: clamped
 *         P: d = -((1 / kinv_t) (cdot_t + bias_t)), impulse += d, apply d along t     (clamp: x < lo ? lo : x > hi ? hi : x: a NaN passes)
 *   - The calls follow the pins', links' and angles' rules word for word.  Checked at add: the pins' body rules, every float finite,
 *     axis.x^2 + axis.y^2 > 2^-20, lower <= upper, hertz >= 0, damping_ratio >= 0, max_force >= 0, hertz > 0 only with lower == upper,
 *     reserved == 0.  set_slider_limits is checked against the slider's stored hertz, set_slider_motors wants finite values and
 *     max_force >= 0; the three setters keep the schedule.
 *   - The other calls, as for angles: remove_bodies / remove_outside drop the sliders of removed bodies and remap the rest; set_state
 *     drops every slider; save / load carry the sliders with their three impulses in HBM; phx_snapshot_export and
 *     phx_snapshot_blob_bytes of a snapshot that holds sliders return PHX_ERR_STATE; set_shard (count > 1), set_comm, reslab and
 *     add_sliders on a sharded world return PHX_ERR_STATE.  A world without sliders allocates and launches exactly what it did without
 *     them. */
typedef struct { int32_t body1, body2;            /* body1: the carriage; body2: the rail, -1 = the world */
                 phx_vec2 anchor1, anchor2;       /* as a pin's; with body2 = -1 anchor2 is a world point */
                 phx_vec2 axis;                   /* the rail's direction in body2's frame (the world: world coordinates); need not be unit length */
                 float lower, upper;              /* on the translation s */
                 float hertz, damping_ratio;      /* > 0 only with lower == upper: a spring towards s = lower */
                 float motor_speed, max_force;    /* max_force > 0: the motor row is on */
                 float impulse, axis_impulse, motor_impulse;   /* accumulated: rows P, L, M; the warm start */
                 uint32_t reserved;               /* 0 */
} phx_slider;                                     /* 72 B */
int  phx_world_add_sliders(phx_world* w, const phx_slider* sliders, int32_t count, int32_t* first);   /* *first (may be NULL) = index of the first new slider */
int  phx_world_remove_sliders(phx_world* w, const int32_t* sliders, int32_t count);
int  phx_world_set_slider_anchors(phx_world* w, const int32_t* sliders, const float* anchors /* 4 per slider: anchor1.x, .y, anchor2.x, .y */, int32_t count);
int  phx_world_set_slider_limits(phx_world* w, const int32_t* sliders, const float* limits /* 2 per slider: lower, upper */, int32_t count);
int  phx_world_set_slider_motors(phx_world* w, const int32_t* sliders, const float* motors /* 2 per slider: motor_speed, max_force */, int32_t count);
int  phx_world_get_sliders(phx_world* w, phx_slider* out, int32_t cap);
int  phx_world_slider_count(phx_world* w, int32_t* count);

/* BREAKS — a joint that gives way: a bridge that collapses, a rope that snaps, a weld that shears.  Every unit of the pin pass (a pin, a
 * link, an angle, a slider) has a break limit L, a float32 with 0 < L <= +inf; a new unit's is +inf: unbreakable.  The test runs on the
 * device behind the pass, the broken unit is removed, and a queue of break events is all that comes down: nothing per step crosses PCIe
 * but a 4-byte count, and the events of a step that has some.  tests/break_spec.py is the definition (scalar float32, every operation
 * rounded on its own, correctly rounded sqrt) and the device matches it byte for byte.
 *   - After the pin pass of a step with time step dt, the impulses the pass stored in the unit's record give its reaction impulse R:
 *         pin     sqrtf(impulse.x impulse.x + impulse.y impulse.y)
 *         link    fabsf(impulse)
 *         angle   fabsf(impulse + motor_impulse)
 *         slider  a = axis_impulse + motor_impulse;  sqrtf(impulse impulse + a a)       (rows P and L, M are orthogonal)
 *     The unit BREAKS in that step iff R > L dt: one float32 product, a strict comparison, false for a NaN.  L is a force for pins, links
 *     and sliders and a torque for angles.  An inactive or idle unit has stored 0 and never breaks.
 *   - A broken unit has acted in the step it broke in: its impulses stay in the velocities and the contacts are solved on them.  Before
 *     the next step's pass it is gone from its list, exactly as if phx_world_remove_<kind> had been called between the two steps: the
 *     others keep their order, indices shift, the schedule is rebuilt (phx_world_pin_schedule_builds counts it).  The library applies
 *     this lazily: at the next step, or at the top of the next call between steps that reads or changes units (the add, remove, set, get
 *     and count calls of each kind, get_pin_schedule, the three calls below, save, remove_bodies / remove_outside).  A step that breaks
 *     something costs what any change of the unit set costs, O(units) bytes; one that breaks nothing 4 bytes.
 *   - Every break is one event; the events of one step are ordered by (kind, index) ascending.  index, body1, body2: the unit's index
 *     in its list and its bodies, in the numbering that held during the step it broke in, before that step's removals.  reaction: R.
 *     threshold: L dt.  step: the ordinal of that step among the steps taken since the previous successful phx_world_break_events (or
 *     since the world was created, restored or loaded), from 0.  Call it once per step: then every event has step 0 and its index is an
 *     index into the lists as they were before the call's step; a caller that lets several steps pass must apply the index shifts of
 *     each step's removals, group by group in step order, to read the later groups' indices.
 *   - phx_world_break_events has phx_world_contact_events' semantics: the events since the last successful call, in step order, then by
 *     (kind, index); *total is always filled; total > cap returns PHX_ERR_CAPACITY and keeps the queue.
 *   - The calls follow the unit calls' rules word for word: between steps only (PHX_ERR_STATE otherwise), everything checked before
 *     anything is queued, PHX_ERR_INVALID leaves the world unchanged, an empty call is a no-op.  Checked: kind in [0, 3], the indices in
 *     range and distinct, no NULL array with count > 0, every limit > 0 and not NaN (+inf is allowed: unbreakable again).
 *     set_break_limits keeps the schedule and tests nothing by itself: a limit below the current load breaks at the next step.
 *   - The other calls: remove_<kind>, remove_bodies and remove_outside carry the limits along with the records they keep; set_state
 *     drops all limits and clears the event queue; save / load carry the limits (a forked world breaks where the original does), and a
 *     load discards what the abandoned timeline had not settled yet and clears the event queue.  A world in which no finite limit was
 *     ever set allocates nothing and launches nothing for this. */
enum { PHX_UNIT_PIN = 0, PHX_UNIT_LINK = 1, PHX_UNIT_ANGLE = 2, PHX_UNIT_SLIDER = 3 };
typedef struct { int32_t kind, index, body1, body2;   /* PHX_UNIT_*; the unit's index in its list and its bodies during the step it broke in */
                 int32_t step;                        /* which step since the previous phx_world_break_events, from 0 */
                 float reaction, threshold;           /* R > threshold = L dt */
                 uint32_t reserved;                   /* 0 */
} phx_break_event;                                    /* 32 B */
int  phx_world_set_break_limits(phx_world* w, int32_t kind, const int32_t* units, const float* limits, int32_t count);
int  phx_world_get_break_limits(phx_world* w, int32_t kind, float* out, int32_t cap);   /* cap >= the kind's count; +inf where none was set */
int  phx_world_break_events(phx_world* w, phx_break_event* out, int32_t cap, int64_t* total);

/* SLEEPING — settled islands rest on the device and wake on touch.  tests/sleep_spec.py is the definition and the device matches it byte
 * for byte.  The contract: a world that sleeps is a world that does not sleep on which somebody applies edits between every two steps:
 * for every body the rule puts to sleep phx_world_set_inverse_masses(body, 0, 0) and phx_world_set_velocities(body, 0, 0, 0), for every
 * body it wakes phx_world_set_inverse_masses(body, its saved values).  A sleeper is a static body to every kernel of the step.
 *   - State per body: asleep, timer (float32), its saved {inv_mass, inv_inertia}.  A body is DYNAMIC iff inv_mass != 0 || inv_inertia != 0,
 *     MOBILE iff dynamic or asleep, AWAKE iff dynamic and not asleep.
 *   - The pass runs once per step on the state the step leaves behind, after IntegratePosition: (1) an awake body with
 *     vx vx + vy vy <= lin lin && w w <= ang ang has timer += dt, every other awake body timer = 0; (2) the edges are the manifolds with
 *     point_count > 0 whose bodies are both mobile and neither a PHX_BODY_SENSOR, and the units of every kind whose bodies are both
 *     mobile (a unit to the world is no edge; a unit that broke in this step still counts in it); (3) components, labelled by their
 *     smallest body; (4) a sleeper is STRUCK if it shares a point_count > 0 manifold with a body that is not mobile and has a nonzero
 *     velocity or angular-velocity word (a conveyor, a kinematic platform); (5) a component with a sleeper and an awake body or a struck
 *     sleeper wakes: masses restored, timer = 0 for all of it; a component without a sleeper whose smallest timer is >= time_to_sleep
 *     sleeps: masses saved and zeroed, velocities +0; anything else stays.  In the step in which something lands on a sleeper the sleeper
 *     still acts as a static; it wakes at that step's end.
 *   - No defaults: the scenes' units are the caller's, so sleeping is off until parameters are set; all three finite and >= 0, else
 *     PHX_ERR_INVALID.  phx_world_set_sleeping(w, NULL) wakes everything, drops the column and turns sleeping off; every mass is then what
 *     it was, byte for byte.  A world that never enabled it launches exactly what it launched before this existed.
 *   - Between steps only (PHX_ERR_STATE otherwise), checked whole before anything is queued; a sharded or communicator-attached world
 *     refuses it, and a world with sleeping enabled refuses to become one.
 *   - phx_world_get_bodies and the other records show a sleeper as the step sees it: inverse masses 0, velocities 0.
 *     phx_world_get_sleep_states shows the body's own masses whether it sleeps or not.
 *   - Every call between steps that names a body or a unit first wakes the sleeping components of the bodies named (a unit names both
 *     of its bodies): add_accelerations, set_velocities, set_poses, set_inverse_masses (the new values then apply), set_body_inverse_mass,
 *     set_body_static, set_collision_filters, set_materials, set_body_flags, remove_bodies / remove_outside (the components that lose a
 *     member, before the compaction), every add_ / remove_ / set_ of pins, links, angles and sliders, and set_break_limits.
 *     phx_world_set_gravity wakes everything.  phx_world_wake_bodies does only that.  New bodies are awake with timer 0; a removal
 *     carries the column along; phx_world_set_state resets it (nobody asleep, the totals 0) and keeps the parameters.
 *   - phx_world_save / phx_world_load with sleeping enabled return PHX_ERR_STATE and change nothing: the snapshot's layout does not carry
 *     the column.  Turn sleeping off first (which wakes everything).
 *   - Queries and contact reports: a sleeper is not static under PHX_QUERY_SKIP_STATIC; a query names no body and wakes nobody.
 *   - phx_world_sleep_counts: the bodies asleep now, and the totals of bodies put to sleep and woken since sleeping was first enabled or
 *     the last phx_world_set_state.
 *   - Cost: one 16-byte column, a handful of launches per step behind IntegratePosition and no host wait of its own: the number of
 *     bodies whose static-ness changed comes down with the next step's joint counts, which is when the schedule needs it. */
typedef struct { float linear_tolerance, angular_tolerance, time_to_sleep; } phx_sleep_params;
int  phx_world_set_sleeping(phx_world* w, const phx_sleep_params* p);   /* NULL: wake everything, drop the column, sleeping off */
int  phx_world_get_sleeping(phx_world* w, phx_sleep_params* out, int32_t* enabled);
typedef struct { int32_t asleep; float timer, inv_mass, inv_inertia; } phx_sleep_state;   /* 16 B; the body's own masses whether asleep or not */
int  phx_world_get_sleep_states(phx_world* w, phx_sleep_state* out, int32_t cap);
int  phx_world_wake_bodies(phx_world* w, const int32_t* bodies, int32_t count);   /* wakes the sleeping component of each listed body */
int  phx_world_sleep_counts(phx_world* w, int32_t* asleep, int64_t* slept_total, int64_t* woken_total);

/* FORCE FIELDS — wind, attractors, drag zones and blasts, computed on the device from the bodies' own state.  tests/field_spec.py is the
 * definition (float32, every operation rounded on its own, IEEE division and square root) and the device matches it byte for byte.  The
 * list is a setting of the world, like gravity: at most PHX_MAX_FIELDS records, applied in list order at the head of every step.
 *   - Who: body i is affected iff inv_mass > 0 (the rule gravity uses, ref: World.cpp:44: static bodies and sleepers are never written)
 *     and category_i & mask != 0, category_i the body's collision-filter category (1 for every body while no filter was ever set).
 *   - Region, tested on the body's centre {x, y}; a NaN centre is outside every shape but ALL.  PHX_REGION_ALL: every body, region = 0.
 *     PHX_REGION_BOX: region = {min.x, min.y, max.x, max.y}, closed: x >= min.x && x <= max.x && y >= min.y && y <= max.y.
 *     PHX_REGION_DISC: region = {c.x, c.y, r, 0}, closed: dx = x - c.x, dy = y - c.y, dx dx + dy dy <= r r.
 *   - PHX_FIELD_UNIFORM: value = {ax, ay, angular, 0}; a = {ax, ay, angular}.
 *     PHX_FIELD_RADIAL: value = {c.x, c.y, strength, falloff_radius}; dx = x - c.x, dy = y - c.y, d = sqrt(dx dx + dy dy); nothing if
 *     !(d > 2^-10); mag = strength, or with falloff_radius > 0: t = 1 - d / falloff_radius, nothing if !(t > 0), mag = strength t;
 *     a = {(dx / d) mag, (dy / d) mag, 0}.  Positive strength pushes away from the centre, negative attracts.
 *     PHX_FIELD_DRAG: value = {flow.x, flow.y, k_lin, k_ang}; c = min(k_lin dt, 1) / dt, ca = min(k_ang dt, 1) / dt;
 *     a = {(flow.x - v.x) c, (flow.y - v.y) c, (0 - w) ca}: the clamp keeps any stiffness from overshooting the flow in one explicit step.
 *     PHX_FIELD_FORCE in flags: the value is a force / torque: a.xy *= inv_mass, a.z *= inv_inertia.
 *   - Sum: accel_i = pending_i + a(field 0) + a(field 1) + ... in list order, every + rounded; pending_i is what
 *     phx_world_add_accelerations or phx_world_set_state left pending, 0 where nothing is.  A field that does not contribute adds
 *     nothing (not + 0).
 *   - When: the pass runs at the head of every step (phx_world_update, phx_world_pre_solve, phx_world_step_begin) with that step's dt, on
 *     the positions and velocities the step starts from, in front of IntegrateVelocity, which consumes the sums as it consumes pending
 *     accelerations; the records' accelerations read zero after the step, as always.  One launch per step whatever the list's length;
 *     a world with an empty list launches nothing and allocates nothing.
 *   - phx_field_check is the single validator (host only, no device): 0 <= count <= PHX_MAX_FIELDS, no NULL array with count > 0; per
 *     field, in this order: a known kind, a known shape, no unknown flag bit, mask != 0, every float finite, box min <= max, disc r >= 0,
 *     the words its shape and kind do not use exactly 0, falloff_radius >= 0, both k >= 0.  The first failure wins: PHX_ERR_INVALID,
 *     named in phx_last_error.
 *   - phx_world_set_fields replaces the whole list (count 0: none) and phx_world_pulse_fields applies one: both call the validator and
 *     leave the world unchanged on failure; between steps only (PHX_ERR_STATE inside pre_solve .. finish_step and step_begin .. step_end);
 *     a sharded or communicator-attached world refuses them (PHX_ERR_STATE), and phx_world_set_shard / set_comm refuse a world whose
 *     list is not empty.  phx_world_get_fields: *count = the list's length, the records into out (PHX_ERR_CAPACITY if cap is smaller).
 *   - The list names no body: phx_world_set_state, phx_world_load, removals and spawns leave it alone, and snapshots do not hold it.
 *     Setting or clearing it changes no joint topology: the cached schedule, the broadphase's splitters and the query / contact indexes stay.
 *   - phx_world_pulse_fields — a blast is a RADIAL pulse with a falloff radius: the velocity change the listed fields would cause in one
 *     step of dt = 1, applied now by the same arithmetic with the velocity as the sum's start: vel_i = vel_i + a(field 0) + a(field 1) + ...
 *     (a DRAG reads the velocity the call found).  Pending accelerations are not touched.  Host-staged bodies are uploaded first, as a removal
 *     uploads them.  Sleepers rest as static bodies and are not affected: a caller that wants a blast to wake a pile calls
 *     phx_world_query_aabb over the blast's extent and phx_world_wake_bodies on the hits first.
 *   - phx_world_apply_impulses is an edit with the edits' rules (EDITS BETWEEN STEPS: indices in range and distinct, checked whole, staged
 *     and queued; every value finite): on a body with inv_mass > 0, r = point - pos, v += inv_mass J, w -= inv_inertia (r.x J.y - r.y J.x) —
 *     the engine's angular velocity is clockwise-positive (tests/pin_spec.py); a static body is skipped.  Like the other edits it wakes
 *     the sleeping components of the bodies it names.
 *   - phx_world_field_passes: the step passes launched so far (pulses do not count). */
#define PHX_MAX_FIELDS 256
enum { PHX_FIELD_UNIFORM = 0, PHX_FIELD_RADIAL = 1, PHX_FIELD_DRAG = 2 };      /* kind  */
enum { PHX_REGION_ALL = 0, PHX_REGION_BOX = 1, PHX_REGION_DISC = 2 };          /* shape */
#define PHX_FIELD_FORCE 1u   /* value is a force / torque: scaled by the body's inverse mass / inverse inertia */
typedef struct { int32_t kind, shape; uint32_t mask, flags; float region[4]; float value[4]; } phx_field;   /* 48 B */
int  phx_field_check(const phx_field* fields, int32_t count);
int  phx_world_set_fields(phx_world* w, const phx_field* fields, int32_t count);
int  phx_world_get_fields(phx_world* w, phx_field* out, int32_t cap, int32_t* count);
int  phx_world_pulse_fields(phx_world* w, const phx_field* fields, int32_t count);
int  phx_world_apply_impulses(phx_world* w, const int32_t* bodies, const float* impulses /* 4 per body: J.x, J.y, point.x, point.y */, int32_t count);
int  phx_world_field_passes(phx_world* w, int64_t* passes);
/* CONTINUOUS BODIES — fast bodies swept so that they cannot tunnel.  IntegratePosition moves a body by dvel + vel*dt in one jump and the
 * broadphase sees only where it lands: a marble of radius 0.25 at 120 units/s covers 2 units per step at 60 Hz and passes a shelf half a
 * unit thick without one manifold ever existing.  A body marked continuous with a core radius rc > 0 is, after each step's
 * IntegratePosition, swept on the device: its core disc {s, rc} is cast along the translation d = e - s the step just gave it (s: the
 * position before the integrator ran, e: after it) against every static body it collides with, and if the disc would have entered one the
 * body is put back to the point of first touch.  The rotation and the velocities stay as the integrator left them; the AABB is recomputed
 * from the new position (UpdateGeom).  The core is strictly smaller than the outline, so a stopped body's outline overlaps the obstacle by
 * at least inradius - rc and the next step's ordinary narrowphase makes the manifold that turns it round.  A world that never named a
 * continuous body launches what it launched before and computes the same bytes.
 *   - phx_world_set_continuous(w, bodies, radii, count): radii[k] > 0 makes body k continuous with that core radius, radii[k] == 0 a
 *     discrete one again.  (A call of its own: phx_world_set_body_flags goes on refusing every bit but PHX_BODY_SENSOR.)  Checked on the
 *     host before anything is queued, PHX_ERR_INVALID otherwise and the world unchanged: indices in range, none twice; every radius finite
 *     and >= 0; rc strictly below the body's inradius about its origin: min(hx, hy) of a box, r of a circle, hy of a capsule,
 *     min_k dot(n_k, v_k) of a polygon (fp32, the stored normals).  phx_continuous_check is that last rule alone (host only, no device):
 *     "<what>: the core radius <rc> of body <b> is not below its inradius <r>".  A later phx_world_set_shapes / phx_world_set_polygons that
 *     would leave a continuous body's rc at or above its new inradius is refused in the same words, the world unchanged.
 *     Between steps only (PHX_ERR_STATE between pre_solve and finish_step); host-staged bodies go up first; PHX_ERR_STATE for a sharded or
 *     communicator-attached world, and a world that holds a continuous body refuses phx_world_set_shard / set_comm / reslab.
 *   - phx_world_get_continuous: every body's core radius in index order, 0 for a discrete body (cap: room for that many).
 *   - The rule (tests/sweep_spec.py is the definition, byte for byte; every operation fp32, rounded on its own).  d = e - s per component;
 *     d == (0, 0): no cast.  A body whose two inverse masses read 0 at the pass (a static body, a sleeper) is never swept, nor is a sensor.
 *     A target is another body whose two inverse masses read 0 when the pass runs (sleepers included), that is no sensor, whose collision
 *     filter passes against the swept body's and that is in no exclusion pair with it: the step's own three tests.  Targets are taken where
 *     they stand when the pass runs: the motion of a static body moved by phx_world_set_poses during the step is not swept.
 *       per target: the circle cast {s, rc, d, max_t = 1} of QUERIES, operation for operation, its AABB conjunct included: a box by its six
 *         parts, a circle body by the disc of radius rc + r, a capsule by its three parts.  tin < 0 (the core overlaps the target at the
 *         start): no hit, the discrete contact owns the pair.  Otherwise t = max(tin, 0) and the normal is the circle cast's.
 *       a polygon target, in its frame (o' = the frame coordinates of s - pos, d' those of d):
 *         start overlap: s_k = dot(n_k, o' - v_k), k the largest, the first on a tie, sm its value; sm <= 0: no hit.  With
 *           e = v_(k+1) - v_k and u = dot(o' - v_k, e): u < 0 picks q = v_k, otherwise u > dot(e, e) picks q = v_(k+1); there h = o' - q
 *           and dot(h, h) < rc*rc: no hit; in the face region sm < rc: no hit.
 *         faces, k in index order: den = dot(n_k, d'); den < 0; t = (dot(n_k, v_k - o') + rc) / den with 0 <= t <= 1; p = o' + d'*t,
 *           u = dot(p - v_k, e_k) with 0 <= u <= dot(e_k, e_k) (the face pushed out by rc, kept to its own extent); normal n_k.
 *         vertices, k in index order: the ray/disc rule about v_k with radius rc, max_t = 1; tin >= 0; normal (nx, ny) / rc.
 *         The smallest t, the first candidate in this order on a tie; the normal through the frame: xv*n.x + yv*n.y.
 *       the skin, skin = rc * 2^-6, enters in two places, and only here.
 *         A target's hit counts only if the step approaches it by more than the skin: dot(normal, d) < -skin.  The smallest t wins, ties
 *         to the lowest target index.
 *         On a hit the body is put back a skin short of the first touch: approach = -dot(normal, d), t' = max(t - skin / approach, 0),
 *         pos = (s.x + d.x*t', s.y + d.y*t'), the AABB by UpdateGeom, and one phx_sweep_hit is recorded, whose t is t'.
 *         Why: the contact rule (SolveJoints) lets a touching pair go on approaching at 0.1 units/s while it is less than 1 unit deep.  A
 *         body put back to the touch itself would start the next step on the touch to a rounding: overlapping by an ulp it would be the
 *         contact's while it may still come on at full speed, touching by an ulp it would be held at t = 0 step after step by that creep,
 *         its sideways motion with it.  A skin short of the touch the next step is decided by what the body does, not by a rounding: one
 *         that still comes on fast is held (t' = 0) until the contact has turned it, one that creeps is let go and sinks into the
 *         contact's care, one that leaves is not approaching.  A creeping body cannot tunnel: it moves less than rc / 64 per step.  The
 *         outline still overlaps the target by inradius - rc - skin where the body stands, so keep rc below inradius / (1 + 2^-6) if the
 *         next step's narrowphase is to find the pair.
 *   - phx_world_sweep_hits: the clamps of the last pass, ascending by body; the list stays on the device and comes down on demand.
 *     *total always receives their number; PHX_ERR_CAPACITY (nothing written) when cap is smaller.  The indices are those of the pass.
 *   - phx_world_sweep_counts: the passes launched and the clamps made since the world was created.  passes stays 0 in a world without a
 *     continuous body, and stops counting when the last one is made discrete.
 *   - The column {rc, s} (16 B per body) exists only once some call named a continuous body.  New bodies are discrete; removals carry the
 *     column; set_state drops it; save / load / fork carry it in HBM; an exported blob carries it as a ninth section {rc, s.x, s.y, 0}
 *     per body behind the baseline, named by column bit 8 and an offset at header byte 112: a blob of a world without the column has
 *     neither and is byte for byte what it was before the bit existed, and such blobs import as they always did.
 *   - Resting bodies, a limit.  The contact rule corrects a penetration only beyond 2 units (SolveJoints' displacement target), so a
 *     body at rest lies up to 2 units inside what it rests on, and a pile that lands drives its lowest bodies in faster than a creep.  A
 *     core that stays clear of that, inradius - rc > 2, is never clamped in a settling pile and the world computes the bytes of its
 *     discrete twin.  A larger core (any body of ordinary size at factor 0.8: marbles.c's marbles) can be clamped while the pile lands
 *     on it: the body is held where its core meets the floor, and from then on the world's bytes are not the discrete twin's.  At
 *     rest a body sinks at 0.1 units/s at most, which is a creep for rc > 0.11 at 60 Hz, and is not held.
 *   - Cost: one wave per continuous body striding over all bodies, O(continuous x bodies) per step: right for tens to thousands of
 *     bullets, wrong for "everything continuous" in a world of 200k bodies.  Routing the pass through the query index is a later change.
 * Out of scope: sweeps against moving bodies, the rotation of the swept body, the core as anything but a disc. */
typedef struct { int32_t body, target; float t; phx_vec2 normal; } phx_sweep_hit;   /* 20 B */
int  phx_continuous_check(const char* what, int32_t body, const phx_shape* shape, const phx_polygon* polygon /* NULL unless shape->kind is PHX_SHAPE_POLYGON */, float rc);
int  phx_world_set_continuous(phx_world* w, const int32_t* bodies, const float* radii, int32_t count);
int  phx_world_get_continuous(phx_world* w, float* out_radii, int32_t cap);
int  phx_world_sweep_hits(phx_world* w, phx_sweep_hit* out, int32_t cap, int64_t* total);
int  phx_world_sweep_counts(phx_world* w, int64_t* passes, int64_t* clamps_total);
/* the measurement (tools/sweep_cost.py): *last_pass_ms (may be NULL) receives the device time of the last pass's kernel that stood between
 * two HIP events, 0 if none did (the call waits for it); then, while `enable` is non-zero, every later pass's kernel is timed so */
int  phx_world_sweep_timing(phx_world* w, int32_t enable, double* last_pass_ms);

int  phx_world_get_solve_stats(phx_world* w, phx_solve_stats* out);
int  phx_world_get_broadphase_stats(phx_world* w, phx_broadphase_stats* out);
/* handles owned by the world (for stage-level queries after an update) */
phx_solver*     phx_world_solver(phx_world* w);
phx_broadphase* phx_world_broadphase(phx_world* w);
/* per-phase wall/device milliseconds of the last update, in World::Update order:
 * 0 IntegrateVelocity 1 UpdateBroadphase 2 UpdatePairs 3 UpdateManifolds 4 PackManifolds
 * 5 RefreshContactJoints 6 SolveJoints 7 IntegratePosition */
int  phx_world_get_phase_ms(phx_world* w, double out8[8]);
/* [min x, max x] over the AABBs of the dynamic bodies, reduced on the device.  An ownership-sharded run (one world per GPU, each
 * holding the islands of one x-slab: phyx_amd/dist.py SlabWorld) checks it against its slab: as long as no body
 * leaves its slab no island can span two ranks and the ranks need nothing from each other but the per-step barrier. */
int  phx_world_x_extent(phx_world* w, float out2[2]);
/* RE-SLAB of an ownership-sharded run (csrc/reslab.hip): the collective hand-over of bodies between the ranks' worlds
 * when a body has reached its slab's boundary.  Every rank calls phx_world_reslab at the same step with the scene indices of its world's
 * bodies (static bodies of the scene live on every rank).  Phase 1: the ranks all-gather {scene index, x-interval} of their dynamic bodies
 * (two bodies that share a manifold cover each other's interval), cut the x axis anew in the gaps no interval covers (phx_reslab_cuts:
 * blocks of overlapping intervals are never split, the cuts balance the body counts) and see whether anybody changes owner; if nobody
 * does, only `bounds` changes (*moved = 0) and the world keeps its allocations, its cached schedule and its broadphase state.  Phase 2,
 * only otherwise: the ranks all-gather their worlds' states (what phx_world_set_state restores, warm-start impulses included) and every
 * rank restores the part of the union world that lives in its new slab (*moved = 1; global_index / *body_count describe the new world).
 * The hand-over is lossless: with unchanged cuts every rank gets its world back byte for byte.
 * Transport: `comm` — the library's RCCL communicator, collectives on device buffers — or, where none can exist (several ranks on one
 * GPU, another process group), the two host callbacks; transport == NULL or size 1: one rank, nothing is exchanged. */
typedef struct {
    int32_t rank, size;
    phx_comm* comm;                                                                        /* may be NULL: the callbacks are used */
    int (*all_gather)(void* user, const void* send, void* recv, size_t bytes_per_rank);  /* host buffers; rank r's share at r * bytes_per_rank; 0 = ok */
    int (*all_reduce_max)(void* user, int64_t* value);                                    /* in place; 0 = ok */
    void* user;
} phx_slab_transport;
int  phx_world_reslab(phx_world* w, const phx_slab_transport* transport, int64_t* global_index, int32_t capacity, int32_t* body_count, int32_t scene_size,
                      double margin, double bounds[2], int32_t* moved);
/* the phases on their own (no device needed for the second and third): this world's dynamic bodies' scene indices and widened x-intervals;
 * every rank's intervals -> sorted by scene index, with the new owner of every body and the ranks' bounds (2 per rank); the cuts themselves */
int  phx_world_reslab_intervals(phx_world* w, const int64_t* global_index, int32_t body_count, int64_t* gi, double* lo, double* hi, int32_t cap, int32_t* count);
int  phx_reslab_plan(int64_t* gi, double* lo, double* hi, int32_t n, int32_t nranks, double margin, int32_t* owner, double* bounds);
int  phx_reslab_cuts(const double* lo, const double* hi, int32_t n, int32_t nranks, double margin, int32_t* owner, double* bounds);
/* diagnostics: [0] steps whose PackManifolds count was settled together with the joint counts (the bet that no manifold dies),
 * [1] those of them that lost the bet (pack run late, joint match repeated), [2] solves repeated because the cached schedule was
 * stale or a group was left uncommitted, [3] third contact points dropped (ref: Collider.cpp:241-242 would overflow) */
int  phx_world_debug_counters(phx_world* w, int64_t out4[4]);
/* diagnostics of the schedule rebuild: [0] rebuilds whose connected components, joint counts and bins came from the MANIFOLDS (made on a
 * side stream while the joint list was refreshed), [1] rebuilds that took them from the joints.  The schedule is the same pure function of
 * the joints either way; PHX_NO_PRELABEL=1 forces [0] to stay 0. */
int  phx_world_build_counts(phx_world* w, int64_t out2[2]);
/* diagnostics of the queries: queue the build of the query index unless it is current for the world's geometry (the queries build it
 * themselves when they take the index path); *builds (may be NULL) = how many times this world has built it */
int  phx_world_query_index(phx_world* w, int64_t* builds);
/* diagnostics of the contacts: queue the build of the contact incidence unless it is current for the world's contact cache (the
 * contacts build it themselves when they take the index path); *builds (may be NULL) = how many times this world has built it.
 * Between steps only, as the contacts. */
int  phx_world_contact_index(phx_world* w, int64_t* builds);
/* per-phase host timers cost one stream synchronisation per phase; off by default (get_phase_ms then returns the last
 * values measured while it was on) */
int  phx_world_set_phase_timing(phx_world* w, int32_t on);

/* ---------------------------------------------------------------------------------------------- */
/* measurement helpers used by bench.py: K solves queued back to back, HIP events on the handle's own stream */
typedef struct {
    double  total_ms;             /* events around the whole timed region                      */
    double  impulse_kernel_ms;    /* sum of the HIP-event brackets around the sweep launches of every 4th step (every step if steps < 8) */
    int64_t impulse_launches;     /* sweep kernels launched by all the steps                    */
    int64_t joint_visits;         /* joints swept by them (skipped joints count as visited)     */
    int64_t impulse_iterations;   /* sweeps executed                                            */
    int64_t bracketed_launches;   /* sweep kernels inside the brackets: impulse_kernel_ms / this = average launch */
} phx_bench_result;
/* runs `steps` solves of identical device-resident input and reports event timings.  Every step needs the input afresh
 * (a solve overwrites velocities and impulses): phx_solver_bench_stage, called BEFORE the caller starts its clock, makes
 * `steps` private copies of (bodies, joints) in HBM and the next bench call on the same arrays solves copy k in step k; without
 * staged copies (or for warm-up steps) a working copy is restored from the caller's arrays in front of every step, inside the
 * timed region (two copy dispatches per step). */
int phx_solver_bench_stage(phx_solver* s, const void* d_bodies, int32_t body_count, const void* d_joints, int32_t joint_count, int32_t steps);
int phx_solver_bench(phx_solver* s, const void* d_bodies, int32_t body_count, const void* d_contact_points,
                     int32_t contact_point_count, const void* d_joints, int32_t joint_count,
                     const phx_config* config, int32_t warmup, int32_t steps, phx_bench_result* out);
/* 64-bit position-sensitive checksum of what the LAST step of the last phx_solver_bench call left in its copy of the input
 * (velocities, displacing velocities, accumulated impulses): identical input + identical schedule => identical checksum, which is
 * how bench.py checks, outside its clock, that the timed solves computed what the warm-up solve computed. */
int phx_solver_bench_checksum(phx_solver* s, uint64_t* out);
/* Same, with a host callback around every step so that a multi-GPU caller can keep its ranks in lock step without the host
 * ever waiting inside the timed region.  hook(user, step, phase) is called
 *   phase 0  right after step `step` has been queued on the handle's stream (phx_solver_stream): start the per-step
 *            exchange here, ordered behind the step on that stream (e.g. an asynchronous RCCL all-reduce);
 *   phase 1  when the rank-local preparation of step `step` (input restore, topology fingerprint) is queued and its sweeps
 *            are not: make the stream wait for the exchange started after step - 1 here, so the exchange overlaps the
 *            preparation.  Called once more with step = `steps` after the last step, to drain the last exchange.
 *   phase 2  only when exchange buffers are set (phx_solver_set_exchange_buffers): step `step` is solved and its results
 *            are packed; run the all-gather of phx_solver_exchange_segment_bytes() on the stream now — the unpack is
 *            queued right after the hook returns.
 * Warm-up steps are numbered -warmup .. -1.  A nonzero return aborts the run with PHX_ERR_STATE. */
typedef int (*phx_step_hook)(void* user, int32_t step, int32_t phase);
int phx_solver_bench_hooked(phx_solver* s, const void* d_bodies, int32_t body_count, const void* d_contact_points,
                            int32_t contact_point_count, const void* d_joints, int32_t joint_count,
                            const phx_config* config, int32_t warmup, int32_t steps, phx_step_hook hook, void* user,
                            phx_bench_result* out);
/* the hipStream_t every launch of this handle goes to (as void*), for callers that order their own work against it */
void* phx_solver_stream(phx_solver* s);

/* raw device memory helpers so callers without a HIP binding (ctypes) can stage resident inputs */
int phx_device_malloc(int device, size_t bytes, void** out);
int phx_device_free(int device, void* p);
int phx_memcpy_h2d(int device, void* dst, const void* src, size_t bytes);
int phx_memcpy_d2h(int device, void* dst, const void* src, size_t bytes);
int phx_memcpy_d2d(int device, void* dst, const void* src, size_t bytes);
/* the same, ordered on `stream` (a hipStream_t such as phx_solver_stream / phx_world_stream): the host-touching copies
 * return when the data has arrived, the device-to-device copy returns when it is queued */
int phx_memcpy_d2h_on(int device, void* dst, const void* src, size_t bytes, void* stream);
int phx_memcpy_h2d_on(int device, void* dst, const void* src, size_t bytes, void* stream);
int phx_memcpy_d2d_on(int device, void* dst, const void* src, size_t bytes, void* stream);
/* diagnostics: with PHX_WAIT_CLOCK=1 in the environment, the time this process has spent waiting for device->host readbacks */
int phx_debug_wait_clock(long long* ns, long long* calls);
/* test entry points of the two device primitives everything else stands on (exclusive scan, radix sort of pairs).  Host arrays go in and
 * come out; each call allocates, copies and synchronises.
 * phx_debug_scan: `nscans` exclusive prefix sums (modulo 2^32) back to back on one stream and one scan scratch.  Scan k covers the next
 *   counts[k] words of `words`; its prefix sums land at the same place of `out`, its sum in totals[k].
 *   loader          0: scanned in place;  1: the words are computed by a loader (read from an array of their own);  2: by a loader that
 *                   also offers 16-byte loads and declines them on every other 4-word base
 *   misalign_words  0 .. 3: how far each scan's device range starts behind a 16-byte boundary
 *   initial_epoch   != 0: the scratch is allocated for the longest scan and its call counter set to this before the first scan
 *                   (< 2^30; the counter starts over when it nears 2^30)
 *   PHX_ERR_STATE when a scan wrote a device word outside its range.
 * phx_debug_radix_sort: one stable sort of n (key, value) pairs; every key must be below 2^bits (bits 0 .. 32).  *which = the buffer
 *   of the ping-pong pair the result ended in (passes & 1).
 * phx_debug_primitive_plan (host only, needs no device): what the two dispatchers choose — the sort's digit width and pass count for
 *   `bits`; for a scan of scan_count words whether it takes the one-workgroup kernel (*scan_single; 0 for an empty scan, which launches
 *   nothing) and its number of 4096-word tiles. */
int phx_debug_scan(int device, const uint32_t* words, const int32_t* counts, int32_t nscans, int32_t loader, int32_t misalign_words,
                   uint32_t initial_epoch, uint32_t* out, uint32_t* totals);
int phx_debug_radix_sort(int device, const uint32_t* keys, const uint32_t* vals, int32_t n, int32_t bits, uint32_t* keys_out,
                         uint32_t* vals_out, int32_t* which);
int phx_debug_primitive_plan(int32_t bits, int32_t scan_count, int32_t* digit_bits, int32_t* passes, int32_t* scan_single,
                             int32_t* scan_tiles);
/* phx_debug_update_manifold (host only, needs no device): UpdateManifolds of ONE pair by the host instantiation of the function the
 * device kernel calls (SHAPES above): the records b1, b2 (pos, xvector, yvector and geom_size are read) with their kinds, the pair's
 * manifold (point_count 0 .. 2 is read and written; the other fields are left alone) and its two contact-point slots pts[0], pts[1],
 * updated in place. */
int phx_debug_update_manifold(const phx_rigid_body* b1, int32_t kind1, const phx_rigid_body* b2, int32_t kind2, phx_manifold* manifold,
                              phx_contact_point pts[2]);
/* ... and the same through the instantiation a world launches once a polygon was named (POLYGONS): a kind may be PHX_SHAPE_POLYGON, whose
 * body's polygon (poly1, poly2; NULL for a body that is none) is stored as the set call stores it, the normals formed from the vertices.
 * A pair without a polygon gives phx_debug_update_manifold's bytes. */
int phx_debug_update_manifold_polygons(const phx_rigid_body* b1, int32_t kind1, const phx_polygon* poly1, const phx_rigid_body* b2, int32_t kind2,
                                       const phx_polygon* poly2, phx_manifold* manifold, phx_contact_point pts[2]);
/* phx_debug_schedule_bins (host only, needs no device): the three host rules every schedule builder shares, on `count` components given by
 * their joint counts sizes[] and unit counts units[] (in body order).  A workgroup shape of L lanes holds L units and 2 L joints.
 *   *lanes            the shape all groups take: big_lanes iff big_lanes != 0 and some non-empty component fits it but not small_lanes
 *   bin_of, rank_of   per component: its bin (-1: an empty component, or one that goes to the HBM group — it fits no workgroup, or
 *                     want_islands is 0) and its rank among the components of its bin
 *   group_offsets     *bins + 1 entries (room for count + 1): the first slot of every bin, then the slots of all bins
 *   *island_count, *island_max_size   GatherIslands' numbers: consecutive components coalesced until a run holds >= 256 joints */
int phx_debug_schedule_bins(const int32_t* sizes, const int32_t* units, int32_t count, int32_t small_lanes, int32_t big_lanes,
                            int32_t want_islands, int32_t* lanes, int32_t* bin_of, int32_t* rank_of, int32_t* group_offsets, int32_t* bins,
                            int32_t* island_count, int32_t* island_max_size);

#ifdef __cplusplus
}
#endif
#endif /* PHYX_AMD_H */
