// island_kernel_body.h — the body of the island kernel (island_kernel.h), included (no include guard, on purpose) by its two kernels: k_solve_islands<T, NB, HALF,
// TRACE> (MAT = false) and k_solve_islands_mat<T, NB> (MAT = true, HALF = TRACE = false).  Both define T, NB, HALF, TRACE and MAT as
// compile-time constants and name their arguments v, iv, bv, joints, cps, ci, pi.  (The body is the kernel's own, not a function the
// kernels call: so written, the plain kernel's gfx950 code is the code it had before materials, instruction for instruction; called
// through a forced-inline function it came out laid out differently, and measurably slower.)
    // body velocities in LDS: float4 {vx, vy, w, tag}, or — fp16 body-state ablation (BASELINE config 5) — four 16-bit
    // words {half vx, half vy, half w, int16 tag}; arithmetic is fp32 either way, HALF rounds on every store
    using BodyT = typename BodyStore<HALF>::type;
    // (record NB of either table belongs to nobody: what a lane would store for a static body goes there — sl1, sl2 below)
    __shared__ BodyT imp[NB + 1];
    __shared__ BodyT disp[NB + 1];
    // static-tag words [imp|disp][parity][body]; during set-up the same 12 KB hold {invMass, invInertia, pos} per body
    // (... and 64 spare words behind them that nobody reads: where a lane that has no static tag to raise sends its atomicMax)
    __shared__ __attribute__((aligned(16))) unsigned sw_raw[4 * NB + 64];
    __shared__ unsigned char is_st[NB];
    // 'some joint was productive in sweep it': slot it % 3; word 3 of either table is never read: an unproductive lane's store goes there
    __shared__ int flag_imp[4], flag_disp[4];
    __shared__ int s_commit;                      // ISL_VERIFY: every workgroup of the launch arrived and none found a difference
    unsigned (*swi)[NB] = reinterpret_cast<unsigned (*)[NB]>(sw_raw);
    unsigned (*swd)[NB] = reinterpret_cast<unsigned (*)[NB]>(sw_raw + 2 * NB);
    float4* par = reinterpret_cast<float4*>(sw_raw);

    const int group = iv.group_list ? iv.group_list[blockIdx.x] : (int)blockIdx.x;
    if (iv.next_ctl && blockIdx.x == 0) {                 // first kernel of its solve: the NEXT solve's control set (two sets alternate)
        if (threadIdx.x < ISL_STAT_SLOTS) { iv.next_visits[threadIdx.x] = 0ull; iv.next_executed[2 * threadIdx.x] = 0; iv.next_executed[2 * threadIdx.x + 1] = 0; }
        if (threadIdx.x == 0) { *iv.next_ctl = 0ull; iv.next_visits[ISL_STAT_SLOTS] = ~0ull; iv.next_visits[ISL_STAT_SLOTS + 1] = 0ull; }
        if (threadIdx.x < STAMP_END_SHARDS) iv.next_visits[ISL_STAT_SLOTS + STAMP_END_BASE + threadIdx.x * STAMP_END_STRIDE] = 0ull;
        if (threadIdx.x < ISL_SHARDS) iv.next_shards[threadIdx.x * ISL_SHARD_STRIDE] = 0ull;
    }
    if (iv.stamp_begin) solve_stamp_begin(v.stamps);      // (no HBM group in front of this launch: it is the solve's first kernel)
    if (iv.ngroups_dev && group >= *iv.ngroups_dev) return;  // (workgroup-uniform, in front of every barrier)
    if (iv.mode == ISL_COMPLETE && iv.done[group] == iv.epoch) return;      // (workgroup-uniform) committed by the launch this one completes
    PHX_ISL_STAMP(0);
    const unsigned long long cycles0 = TRACE ? __builtin_readcyclecounter() : 0ull;
    // TRACE: per wave, shader cycles spent in class steps {working: in the unit update, then at the barrier; idle: whole step}
    unsigned long long tw_work = 0, tw_bar = 0, tw_idle = 0, tw_work_big = 0; unsigned tw_nwork = 0, tw_nidle = 0, tw_nbig = 0;
    const int tid = threadIdx.x;

    // Set-up is two dependent HBM round trips: level 1 = the group's descriptor, the lane's unit record and its body ids (all at
    // addresses that depend on the group number only), level 2 = the body records, the joints and the contact points.
    // EVERY request of both levels is unconditional — a lane without a unit asks for joint 0 and its contact point, a lane without a
    // body for body 0, and throws the answer away: a request under a branch is waited for at the join with `s_waitcnt vmcnt(0)`
    // (loads return in order, and the compiler cannot count what a branch may have skipped), which made level 2 THREE round trips:
    // the joints were asked for only when the body records were back, the follower's contact point only when the leader's was.
    static_assert(NB % T == 0, "a lane owns NB / T whole body slots");
    constexpr int BI = NB / T;                             // body records per lane
    int body_id[BI];
#pragma unroll
    for (int k = 0; k < BI; ++k) body_id[k] = iv.bodies[(size_t)group * NB + tid + k * T];      // (entries past the group's count: unused words of its table)
    const int4 ua = iv.unit_recs[2 * ((size_t)group * T + tid)], ub = iv.unit_recs[2 * ((size_t)group * T + tid) + 1];
    const int4 d = iv.desc[group];
    const int units_word = iv.units[group];
    if (TRACE) { __builtin_amdgcn_s_waitcnt(0x0F70); PHX_ISL_PHASE(0); }      // (diagnostic build only: level 1 is back)
    // (schedule.h LANES: the classes' lane ranges sit on wave boundaries where the lanes allow it — a lane has a unit or it has not)
    const int ncol = island_word_classes(units_word), nstatic = island_word_static(units_word);
    const bool live = ua.x >= 0;
    const bool has2 = live && ua.y >= 0;
    const int jid0 = live ? ua.x : 0, jid1 = has2 ? ua.y : 0;
    const unsigned loc = live ? (unsigned)ub.x : 0u;
    const int col = live ? ub.y : -1;
    const int l1 = (int)(loc & 0xFFFFu), l2 = (int)(loc >> 16);
    const bool verify = iv.mode == ISL_VERIFY;             // (launch-uniform)
    // level 2, in the order its addresses become known: the joints and the contact points hang on `ua` alone ...
    // (the contact point index is part of the topology the schedule was built — and is gated — for: ua.z == j.contact_point_index)
    const phx_contact_joint j = joints[jid0], jf = joints[jid1];
    const float4* const cpa = reinterpret_cast<const float4*>(&cps[clamp_index(live ? ua.z : 0, v.ncp)]);   // 32-byte records
    const float4* const cpb = reinterpret_cast<const float4*>(&cps[clamp_index(has2 ? ua.w : 0, v.ncp)]);
    const float4 cpa0 = cpa[0], cpb0 = cpb[0];
    const float2 nna = *reinterpret_cast<const float2*>(cpa + 1), nnb = *reinterpret_cast<const float2*>(cpb + 1);
    // ... the body records on the body ids and the group's body count
#pragma unroll
    for (int k = 0; k < BI; ++k) if (tid + k * T >= d.w) body_id[k] = -1;
    float4 rec_imp[BI], rec_disp[BI], rec_par[BI];
    float2 rec_mat[BI];
#pragma unroll
    for (int k = 0; k < BI; ++k) {                         // the resident arrays ARE PrepareBodies' staged form
        const int b = body_id[k] < 0 ? 0 : body_id[k];     // (ref: Solver.cpp:456-480; body_view.h): three coalesced 16-byte loads
        rec_imp[k] = bv.vel[b]; rec_imp[k].w = __int_as_float(-1);
        rec_disp[k] = bv.dvel[b]; rec_disp[k].w = __int_as_float(-1);
        rec_par[k] = bv.mpos[b];
        if (MAT) rec_mat[k] = view_material<MAT>(v, b);    // (and the body's material: one 8-byte load)
    }
    // ISL_VERIFY: the unit record against the joint it points at (the body ids: two more words of the group's table, L2-warm)
    int g1 = 0, g2 = 0;
    if (verify) { g1 = iv.bodies[(size_t)group * NB + l1]; g2 = iv.bodies[(size_t)group * NB + l2]; }
    if (tid < 3) { flag_imp[tid] = 0; flag_disp[tid] = 0; }

    IslJoint q0{}, q1{};
    float4 da0 = make_float4(0.f, 0.f, 0.f, 0.f), da1 = da0;     // delta1, delta2 of the two contact points
    bool differs = false;                                  // ISL_VERIFY: the schedule was built for other joints / other static bodies
    if (live) {                                            // PrepareJoints (ref: Solver.cpp:509-521)
        da0 = cpa0;
        q0.nx = nna.x; q0.ny = nna.y;
        q0.accN = j.normal_accumulated_impulse; q0.accF = j.friction_accumulated_impulse;
        if (verify) {
            differs = j.contact_point_index != ua.z || j.body1 != g1 || j.body2 != g2;
            if (has2) differs |= jf.contact_point_index != ua.w || jf.body1 != g1 || jf.body2 != g2;
        }
    }
    if (has2) {
        da1 = cpb0;
        q1.nx = nnb.x; q1.ny = nnb.y;
        q1.accN = jf.normal_accumulated_impulse; q1.accF = jf.friction_accumulated_impulse;
    }
    if (TRACE) { __builtin_amdgcn_s_waitcnt(0x0F70); PHX_ISL_PHASE(1); }      // (diagnostic build only: level 2 is back, nothing of it used yet)
#pragma unroll
    for (int k = 0; k < BI; ++k) {
        if (body_id[k] < 0) continue;
        const int i = tid + k * T;
        body_store(imp, i, rec_imp[k]);
        if (MAT) body_store(disp, i, make_float4(rec_mat[k].x, rec_mat[k].y, 0.f, 0.f));      // (until the refresh has read it)
        else body_store(disp, i, rec_disp[k]);
        par[i] = rec_par[k];
        const bool st = rec_par[k].x == 0.f && rec_par[k].y == 0.f;
        is_st[i] = st ? 1 : 0;
        differs |= st != (i < nstatic);                    // (the builders list a group's static bodies first)
    }
    // Level 2 is back, whole, in every mode (the refresh behind the barrier needs all of it): said here, in front of the arrival, so
    // that no later wait for a load — it would be `vmcnt(0)`, the counter is one and in order — also waits for the arrival's answer.
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
    unsigned long long arrived_before = 0ull;              // (lane 0) what the shard counter read when this workgroup arrived
    unsigned my_arrival = 1u;
    PHX_ISL_PHASE(2);
    if (verify) {
        // ARRIVE: this workgroup has compared everything it owns.  One device-scope atomic carries the arrival and the verdict, so
        // whoever sees all arrivals also sees every verdict (island_view.h).  The returned value is looked at behind PreStep:
        // nothing waits for this round trip.
        const int any = __syncthreads_or(differs ? 1 : 0);
        my_arrival = any ? 1u + ISL_BAD : 1u;
        if (tid == 0) {
            // (the index goes through a vector register on purpose: on a wave-uniform address the compiler's atomic optimiser
            //  combines the wave's lanes and reads the returned value back with v_readfirstlane at once — `s_waitcnt vmcnt(0)`
            //  right behind the atomic, a device-scope round trip in front of the barrier every wave of the group waits at)
            int shard = ((int)blockIdx.x % ISL_SHARDS) * ISL_SHARD_STRIDE;
            asm volatile("" : "+v"(shard));
            arrived_before = atomicAdd(&iv.shards[shard], (unsigned long long)my_arrival);
        }
    } else __syncthreads();
    PHX_ISL_STAMP(1);
    float im1 = 0.f, ii1 = 0.f, im2 = 0.f, ii2 = 0.f;
    float mu = 0.3f;                                       // the unit's friction coefficient (kFrictionCoefficient unless MAT)
    if (live) {
        const float4 p1 = par[l1], p2 = par[l2];           // {im, ii, pos.x, pos.y} of the two bodies
        if (MAT) {
            const float4 m1 = body_load(disp, l1), m2 = body_load(disp, l2);
            const float2 a = make_float2(m1.x, m1.y), b = make_float2(m2.x, m2.y);
            mu = material_mu(a, b);
            const float e = material_e(a, b);
            float4 V1 = float4{}, V2 = float4{};
            if (e != 0.f) { V1 = body_load(imp, l1); V2 = body_load(imp, l2); }      // (the solve's velocities: stored behind the barrier above)
            refresh_joint<true>(q0, da0.x, da0.y, da0.z, da0.w, p1, p2, e, V1, V2);
            if (has2) refresh_joint<true>(q1, da1.x, da1.y, da1.z, da1.w, p1, p2, e, V1, V2);
        } else {
            refresh_joint(q0, da0.x, da0.y, da0.z, da0.w, p1, p2);
            if (has2) refresh_joint(q1, da1.x, da1.y, da1.z, da1.w, p1, p2);
        }
        im1 = p1.x; ii1 = p1.y; im2 = p2.x; ii2 = p2.y;
    }
    // THE DISPLACEMENT HALF OF A GROUP THAT HAS NOTHING TO PUSH APART IS A NO-OP, bit for bit: if every displacing velocity of the group
    // is +0, no joint is deeper than the allowed penetration (dstD = +0, ref: Solver.cpp:672-680) and everything a visit multiplies is
    // finite, then a visit (ref: Solver.cpp:960-1005) computes dv = +0 - (+-0) ... = +0, di = max(+-0, -accD = -0) = -0, adds (finite x -0)
    // to +0 velocities (= +0) and -0 to accD = +0 (= +0), and is not productive — in either arithmetic form.  So the reference's first
    // displacement sweep finds nothing productive and is its last (ref: Solver.cpp:210); the group skips it and reports the one sweep
    // (a resting stack's every solve: 1.5 us of cfg 2's launch).
    auto finite_bits = [](float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; };
    auto joint_quiet = [&](const IslJoint& q) {
        return __float_as_uint(q.dstD) == 0u && finite_bits(q.nx) && finite_bits(q.ny) && finite_bits(q.aN1) && finite_bits(q.aN2) && finite_bits(q.cimN)
               && finite_bits(im1) && finite_bits(ii1) && finite_bits(im2) && finite_bits(ii2);
    };
    bool stirs = live && !(joint_quiet(q0) && (!has2 || joint_quiet(q1)));
#pragma unroll
    for (int k = 0; k < BI; ++k)
        if (body_id[k] >= 0) stirs |= (__float_as_uint(rec_disp[k].x) | __float_as_uint(rec_disp[k].y) | __float_as_uint(rec_disp[k].z)) != 0u;
    PHX_ISL_PHASE(3);
    const bool disp_quiet = __syncthreads_or(stirs ? 1 : 0) == 0;      // (the barrier that was here anyway)
    if (MAT) {                                             // the materials are read: the displacing velocities take their place
#pragma unroll
        for (int k = 0; k < BI; ++k) if (body_id[k] >= 0) body_store(disp, tid + k * T, rec_disp[k]);
    }
#pragma unroll
    for (int k = 0; k < BI; ++k) par[tid + k * T] = make_float4(0.f, 0.f, 0.f, 0.f);      // the parameter table is dead: now the tag words (all zero bits)
    const bool st1 = (im1 == 0.f && ii1 == 0.f), st2 = (im2 == 0.f && ii2 == 0.f);
    const bool wave_static = __any(live && (st1 || st2));      // (wave-uniform, fixed for the solve)
    int sm1 = st1 ? -1 : 0, sm2 = st2 ? -1 : 0;                // (as masks: the hot form selects with them instead of branching)
    asm volatile("" : "+v"(sm1), "+v"(sm2));
    // A static body's record is never stored.  Said with the ADDRESS, not with a predicate: a lane stores both records of its unit
    // in every step, a static one into the spare record NB.  (As `if (!st1) store; if (!st2) store` the end of a class step — the
    // one stretch between a wave's last FMA and the barrier everybody waits at — was two exec regions with two taken branches.)
    const int sl1 = st1 ? NB : l1, sl2 = st2 ? NB : l2;
    __syncthreads();
    PHX_ISL_STAMP(2);

    // PreStepJoints (ref: Solver.cpp:736-750), class by class: leader, then follower
    for (int c = 0; c < ncol; ++c) {
        if (col == c) {
            float4 B1 = body_load(imp, l1), B2 = body_load(imp, l2);
            prestep_joint(q0, q0.accN, q0.accF, B1, B2, im1, ii1, im2, ii2, false, false);
            if (has2) {
                if (HALF) { B1 = body_round<HALF>(B1); B2 = body_round<HALF>(B2); }      // (the ablation rounds on every joint's store)
                prestep_joint(q1, q1.accN, q1.accF, B1, B2, im1, ii1, im2, ii2, false, false);
            }
            body_store(imp, sl1, B1);
            body_store(imp, sl2, B2);
        }
        __syncthreads();
        if (TRACE && c < 4) PHX_ISL_PHASE(4 + c);
    }

    if (verify && tid == 0) {
        // the last arriver of a shard forwards the shard's verdict to the solve's control word
        // (both halves of the answer stay reserved until here: a register of a load in flight that is given to another value is
        //  waited for where that value is written — the high half is dead, and was, at the head of the refresh)
        asm volatile("" : "+v"(arrived_before));
        const unsigned now = (unsigned)arrived_before + my_arrival;
        const unsigned shard = blockIdx.x % ISL_SHARDS, want = (iv.nexpect - shard + ISL_SHARDS - 1) / ISL_SHARDS;
        if ((now & ISL_ARRIVE_MASK) == want) atomicAdd(iv.ctl, now >= ISL_BAD ? (unsigned long long)(1u + ISL_BAD) : 1ull);
    }
    PHX_ISL_STAMP(3);
    int done_imp = 0, done_disp = (pi > 0 && disp_quiet) ? 1 : 0;      // (a quiet group's one displacement sweep: see above)
    bool imp_alive = ci > 0, disp_alive = pi > 0 && !disp_quiet;
    const int iters = ci > pi ? ci : pi;
    unsigned early_ctl = 0u;                               // (lane 0) the control word as read a few sweeps in: by then every workgroup has long arrived
    int it = 0, c = 0, slot = 0;                           // the sweep, the class and the flag slot the step forms below work on
    // ISL_VERIFY: look at the control word a few sweeps in, off the critical path (the load returns while the sweeps run); the commit
    // decision at the end then needs no memory round trip of its own unless some workgroup really is that late
    auto peek_ctl = [&]() { if (verify && it == 3 && tid == 0 && iv.wait_polls > 0) early_ctl = (unsigned)__hip_atomic_load(iv.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // three flag slots in rotation: the one cleared for the next sweep was read last at the end of sweep it - 2, and every class
    // step of sweep it - 1 has put a barrier in between — so a sweep needs no barrier of its own at its end
    auto next_slot = [&]() { slot = it % 3; if (tid == 0) { const int next = slot == 2 ? 0 : slot + 1; flag_imp[next] = 0; flag_disp[next] = 0; } };
    // TRACE level 2 (phx_solver_set_trace: per-wave cycle counts of every class step — ~15 % slower)
    const bool wt = TRACE && iv.wave_trace;
    unsigned long long ts0 = 0ull, ts1 = 0ull; bool working = false;
    // ... and, in the impulse-only loop, where a working wave's step goes (island_view.h ISL_PHASE_WORDS; what the wave's FIRST lane saw:
    // a step in which that lane has no unit of the class, or was left out by the skip test, is not counted): barrier released -> LDS data
    // back (tp1) -> last FMA (tp2) -> stores issued (tp3) -> lgkmcnt(0) (ts1) -> barrier released; a step the skip test left out counts apart
    unsigned tp1 = 0u, tp2 = 0u, tp3 = 0u, in_step[5] = {0u, 0u, 0u, 0u, 0u};      // (32-bit: the differences are what counts)
    unsigned in_n = 0u;
    auto step_begin = [&]() { if (wt) { ts0 = __builtin_readcyclecounter(); working = __any(col == c); tp3 = 0u; } };
    auto step_work_done = [&]() { if (wt) { __builtin_amdgcn_s_waitcnt(0xC07F); ts1 = __builtin_readcyclecounter(); } };      // lgkmcnt(0): the barrier's own wait
    auto step_end = [&](const bool hot) {
        if (!wt) return;
        const unsigned long long ts2 = __builtin_readcyclecounter();
        if (working && hot && tp3)
            { in_step[0] += tp1 - (unsigned)ts0; in_step[1] += tp2 - tp1; in_step[2] += tp3 - tp2; in_step[3] += (unsigned)ts1 - tp3; in_step[4] += (unsigned)(ts2 - ts1); ++in_n; }
        if (working) {
            if (__popcll(__ballot(col == c)) > 32) { tw_work_big += ts1 - ts0; ++tw_nbig; } else { tw_work += ts1 - ts0; ++tw_nwork; }
            tw_bar += ts2 - ts1;
        } else { tw_idle += ts2 - ts0; ++tw_nidle; }
    };
    // A CLASS STEP of one sweep half (IMP: the impulses on the velocities, ref: Solver.cpp:790-896; else the displacement on the displacing
    // velocities, ref: Solver.cpp:960-1005) for the lane's unit: both body records in one LDS round trip, ONE skip test per unit — the
    // follower's test equals its leader's: a skipped leader changes no tag, and an evaluated one either leaves the tags as they were or
    // raises them to `it` — and one tag update; straight-line but for the follower's mask: a class step is one wave's instruction
    // stream, and every taken branch in it is ~20 cycles.  `ws` = some unit of the wave touches a static body (wave-uniform, fixed for
    // the solve): only then the static tags are looked up and raised (they are class-synchronous: solver_kernels.h), the static records
    // restored between the joints (a static body's record is never stored: the follower must see it untouched); what the unit would
    // store for them goes to the spare record (sl1, sl2).
    // (Rounds 2-4 had a general form beside this one — a skip test and a tag update per joint, two dependent LDS round trips — which
    //  every first sweep still took: same results, ~2.5 x the cycles.)
    auto half_step = [&](auto IMPC, const bool ws) {
        constexpr bool IMP = decltype(IMPC)::value;
        BodyT* const rec = IMP ? imp : disp;
        unsigned (*const sw)[NB] = IMP ? swi : swd;
        float4 B1 = body_load(rec, l1), B2 = body_load(rec, l2);
        // (`ws`: the static tags' words travel with the body records — every lane of the wave reads them, a dynamic body's
        //  are zero — instead of two more dependent LDS round trips for the one lane that needs them.  Both parities of both bodies,
        //  at addresses fixed for the solve: which of the two is sweep it's table is said by the thresholds below, on the scalar unit)
        unsigned e1 = 0u, o1 = 0u, e2 = 0u, o2 = 0u;
        if (ws) { e1 = sw[0][l1]; o1 = sw[1][l1]; e2 = sw[0][l2]; o2 = sw[1][l2]; }
        // (everything in ONE LDS round trip: left alone, the compiler reads the two tags, tests, and only then — under the
        //  branch — the six velocity words: two dependent round trips on the critical path of every class step)
        // (`ws`: the records are inputs of the fence, not tied in-and-out operands: tied, the eight words were copied to other
        //  registers in front of the leader, which writes its results beside them anyway — the follower's static body wants them back)
        if (!HALF && !ws) asm volatile("" : "+v"(B1.x), "+v"(B1.y), "+v"(B1.z), "+v"(B1.w), "+v"(B2.x), "+v"(B2.y), "+v"(B2.z), "+v"(B2.w));
        if (!HALF && ws) asm volatile("" : "+v"(e1), "+v"(o1), "+v"(e2), "+v"(o2) : "v"(B1.x), "v"(B1.y), "v"(B1.z), "v"(B1.w), "v"(B2.x), "v"(B2.y), "v"(B2.z), "v"(B2.w));
        if (HALF && ws) asm volatile("" : "+v"(e1), "+v"(o1), "+v"(e2), "+v"(o2));
        if (wt) { __builtin_amdgcn_s_waitcnt(0xC07F); tp1 = (unsigned)__builtin_readcyclecounter(); }
        bool active = max(__float_as_int(B1.w), __float_as_int(B2.w)) > it - 2;
        if (ws) {
            // solver_kernels.h static_productive on the words already here, as two unsigned compares per table.  The words only grow
            // (atomicMax), sweep s raises table s & 1 to static_word(s, class) = (s + 1) << 16 | 0xFFFF - class, so in sweep `it` the
            // other table holds at most it << 16 | 0xFFFF and this one at most (it + 1) << 16 | 0xFFFF:
            //   'raised in sweep it - 1' (high half == it; always in sweep 0)             <=>  word >= it << 16
            //   'raised in this sweep by an earlier class' (high half == it + 1, class < c) <=>  word > static_word(it, c)
            // And no select between this test and the body's own tag is needed: a static body's record is never stored, its tag
            // stays -1 and passes `> it - 2` in sweep 0 only, where the static test passes too; a dynamic body's words stay zero
            // and pass the static test in sweep 0 only, where its tag (-1) passes too.  So the four tests are simply OR-ed.
            const unsigned prev = (unsigned)it << 16, cur = static_word(it, c) + 1u;
            const unsigned te = (it & 1) ? prev : cur, to = (it & 1) ? cur : prev;
            active |= max(e1, e2) >= te;
            active |= max(o1, o2) >= to;
        }
        if (active) {
            const float4 S1 = B1, S2 = B2;
            bool prod = IMP ? impulse_productive(impulse_visit(q0, q0.accN, q0.accF, B1, B2, im1, ii1, im2, ii2, mu))
                             : displacement_productive(displacement_visit(q0, q0.accD, B1, B2, im1, ii1, im2, ii2));
            if (has2) {
                if (HALF) { B1 = body_round<HALF>(B1); B2 = body_round<HALF>(B2); }      // (the ablation rounds on every joint's store)
                if (ws) {      // (a visit leaves the tag word alone: three words a body)
                    B1.x = sm1 ? S1.x : B1.x; B1.y = sm1 ? S1.y : B1.y; B1.z = sm1 ? S1.z : B1.z;
                    B2.x = sm2 ? S2.x : B2.x; B2.y = sm2 ? S2.y : B2.y; B2.z = sm2 ? S2.z : B2.z;
                }
                prod |= IMP ? impulse_productive(impulse_visit(q1, q1.accN, q1.accF, B1, B2, im1, ii1, im2, ii2, mu))
                             : displacement_productive(displacement_visit(q1, q1.accD, B1, B2, im1, ii1, im2, ii2));
            }
            if (wt) { asm volatile("" : "+v"(B1.x), "+v"(B1.y), "+v"(B1.z), "+v"(B2.x), "+v"(B2.y), "+v"(B2.z)); tp2 = (unsigned)__builtin_readcyclecounter(); }
            // The tail, straight-line and stores first: the velocity words are final at the last FMA, and `prod` hangs on the impulses
            // alone, so the tag select sits under the last FMAs.  What only a productive lane does is said with the ADDRESS (as sl1,
            // sl2 are): the sweep's flag goes to the slot or to the table's spare word, a static tag to the body's word or to a
            // spare word of the lane's own — no exec region and no taken branch between the last FMA and the barrier.
            B1.w = prod ? __int_as_float(it) : B1.w; B2.w = prod ? __int_as_float(it) : B2.w;
            body_store(rec, sl1, B1);
            body_store(rec, sl2, B2);
            (IMP ? flag_imp : flag_disp)[prod ? slot : 3] = 1;
            if (ws) {
                const int tab = (IMP ? 0 : 2 * NB) + (it & 1) * NB, spare = 4 * NB + (tid & 63);
                atomicMax(&sw_raw[(prod && st1) ? tab + l1 : spare], static_word(it, c));
                atomicMax(&sw_raw[(prod && st2) ? tab + l2 : spare], static_word(it, c));
            }
            if (wt) tp3 = (unsigned)__builtin_readcyclecounter() | 1u;
        }
    };
    const std::true_type IMPULSES{}; const std::false_type DISPLACEMENT{};
    // The sweeps, in two loops: both halves while the displacement half still runs (the displacement sweeps of a resting scene end
    // after the first: nothing is deeper than the allowed penetration, ref: Solver.cpp:672-680, 210), then the impulses alone — once
    // over, the displacement sweeps stay over (disp_alive only falls, `it` only grows).  (One loop for both cost the impulse-only step
    // a dozen register copies: the displacement accumulators' values flowed through its exits.)
    bool hot_from_here = false;
    for (; it < iters; ++it) {
        const bool imp_on = imp_alive && it < ci, disp_on = disp_alive && it < pi;
        if (!imp_on && !disp_on) break;
        if (imp_on && !disp_on) { hot_from_here = true; break; }
        peek_ctl();
        next_slot();
        for (c = 0; c < ncol; ++c) {
            step_begin();
            if (col == c) {
                if (wave_static) {
                    if (imp_on) half_step(IMPULSES, true);
                    if (disp_on) half_step(DISPLACEMENT, true);
                } else {
                    if (imp_on) half_step(IMPULSES, false);
                    if (disp_on) half_step(DISPLACEMENT, false);
                }
            }
            step_work_done();
            __syncthreads();
            step_end(false);
        }
        if (imp_on) { done_imp = it + 1; imp_alive = flag_imp[slot] != 0; }        // (behind the last class step's barrier)
        if (disp_on) { done_disp = it + 1; disp_alive = flag_disp[slot] != 0; }
        if (TRACE && it == 0) PHX_ISL_PHASE(8);
    }

    // (a loop of its own for either kind of wave — wave_static is wave-uniform and fixed, every wave passes the same barriers: with
    //  both forms of the step in one loop the unit's accumulators were copied between the registers of the two forms, eight moves
    //  between the stores and the barrier in every step, and every step began with a branch on wave_static)
    auto hot_sweeps = [&](const bool ws) {
        for (; it < ci && imp_alive; ++it) {
            peek_ctl();
            next_slot();
            for (c = 0; c < ncol; ++c) {
                step_begin();
                if (col == c) half_step(IMPULSES, ws);
                step_work_done();
                __syncthreads();
                step_end(true);
            }
            done_imp = it + 1; imp_alive = flag_imp[slot] != 0;
            if (TRACE && it == 0) PHX_ISL_PHASE(8);
        }
    };
    if (hot_from_here) { if (wave_static) hot_sweeps(true); else hot_sweeps(false); }

    PHX_ISL_STAMP(4);
    // results go straight back into the caller's records (commit-gated like k_finish_*); the refreshed constants
    // never leave the registers
    if (verify) {
        // every workgroup of the launch is resident at once (the host launches ISL_VERIFY only then), so by now — tens of
        // microseconds after its own arrival — all of them have arrived and this wait is one load; it is BOUNDED all the same: if
        // it runs out (a GPU shared with somebody else's kernels) the group stays uncommitted and the host completes it (ISL_COMPLETE)
        if (tid == 0) {
            const unsigned shards = iv.nexpect < (unsigned)ISL_SHARDS ? iv.nexpect : (unsigned)ISL_SHARDS;
            unsigned lo = early_ctl;
            int polls = 0;
            const bool settled = (lo & ISL_ARRIVE_MASK) >= shards || lo >= ISL_BAD;      // (complete, or spoiled: both final)
            for (; !settled && polls < iv.wait_polls; ++polls) {
                lo = (unsigned)__hip_atomic_load(iv.ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((lo & ISL_ARRIVE_MASK) >= shards || lo >= ISL_BAD) break;
                __builtin_amdgcn_s_sleep(32);
            }
            s_commit = lo == shards ? 1 : 0;
            if (!settled && polls == iv.wait_polls) atomicOr(iv.ctl, ISL_TIMEOUT);      // (nobody may take this solve for complete)
        }
        __syncthreads();
        PHX_ISL_PHASE(9);
        if (!s_commit) { if (iv.stamp_end) solve_stamp_end(v.stamps); return; }
    } else if (iv.mode == ISL_GATED && *v.fingerprint != v.expected_fingerprint) { if (iv.stamp_end) solve_stamp_end(v.stamps); return; }
    if (live) {                                            // FinishJoints (ref: Solver.cpp:543-544)
        phx_contact_joint& out = joints[jid0];
        __builtin_nontemporal_store(q0.accN, &out.normal_accumulated_impulse);
        __builtin_nontemporal_store(q0.accF, &out.friction_accumulated_impulse);
    }
    if (has2) {
        phx_contact_joint& out = joints[jid1];
        __builtin_nontemporal_store(q1.accN, &out.normal_accumulated_impulse);
        __builtin_nontemporal_store(q1.accF, &out.friction_accumulated_impulse);
    }
    // FinishBodies (ref: Solver.cpp:488-492), dynamic bodies only.  A group whose displacement half was skipped (disp_quiet, above)
    // leaves its displacing velocities alone: by that proof every word of them is the +0 it loaded, and the fourth word is 0 in
    // every record (body_view.h) — the stores would put back, bit for bit, what is there (cfg 2: every group, 3.1 MB a launch).
    if (disp_quiet) {                                      // (workgroup-uniform)
#pragma unroll
        for (int k = 0; k < BI; ++k) {
            const int i = tid + k * T;
            if (body_id[k] < 0 || is_st[i]) continue;
            const float4 a = body_load(imp, i);
            store_nt(&bv.vel[body_id[k]], a.x, a.y, a.z, 0.f);
        }
    } else {
#pragma unroll
        for (int k = 0; k < BI; ++k) {
            const int i = tid + k * T;
            if (body_id[k] < 0 || is_st[i]) continue;
            const float4 a = body_load(imp, i), e = body_load(disp, i);
            store_nt(&bv.vel[body_id[k]], a.x, a.y, a.z, 0.f);
            store_nt(&bv.dvel[body_id[k]], e.x, e.y, e.z, 0.f);
        }
    }
    if (iv.stamp_end) solve_stamp_end(v.stamps);           // (no HBM group behind this launch: it is the solve's last kernel)
    if (tid == 0) {
        if (iv.mode != ISL_GATED) iv.done[group] = iv.epoch;      // committed
        const int slot = group % ISL_STAT_SLOTS;
        atomicMax(&iv.executed[2 * slot], done_imp);
        atomicMax(&iv.executed[2 * slot + 1], done_disp);
        atomicAdd(&iv.visits[slot], (unsigned long long)done_imp * (unsigned long long)d.y);
    }
    if (TRACE && iv.wave_trace && (tid & 63) == 0) {
        unsigned long long* w = iv.wave_trace + ((size_t)group * (T / 64) + (tid >> 6)) * 8;
        w[0] = tw_work; w[1] = tw_bar; w[2] = tw_idle; w[3] = ((unsigned long long)tw_nwork << 32) | tw_nidle; w[4] = tw_work_big; w[5] = tw_nbig;
        w[6] = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));        // HW_REG_HW_ID: wave, SIMD, pipe, CU, SH, SE ... (tools/simd_map.py)
        w[7] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 0xF;  // XCC id
        if (iv.phase_trace) {
            unsigned long long* p = iv.phase_trace + (size_t)group * ISL_PHASE_WORDS + 16 + (tid >> 6) * 8;
#pragma unroll
            for (int k = 0; k < 5; ++k) p[k] = in_step[k];
            p[5] = in_n; p[6] = wave_static ? 1ull : 0ull;
        }
    }
    if (TRACE) {
        PHX_ISL_PHASE(10);
        __builtin_amdgcn_s_waitcnt(0);         // the stores above have left the wave
        PHX_ISL_STAMP(5);
        if (tid == 0) {
            iv.trace[(size_t)group * 8 + 6] = (unsigned long long)(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & 0xF)    // HW_REG_XCC_ID[3:0]
                                              | ((__builtin_readcyclecounter() - cycles0) << 4);                                  // + s_memtime ticks start -> end
            iv.trace[(size_t)group * 8 + 7] = ((unsigned long long)ncol << 32) | (unsigned)done_imp;
        }
    }
