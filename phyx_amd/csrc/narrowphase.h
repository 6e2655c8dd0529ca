// narrowphase.h — box/box SAT, contact generation and manifold merging as __host__ __device__ functions.
//
// This is the step between the two hot halves of the path; it restates
// ref: src/Collider.cpp:8-245 and src/Geom.h:10-85 on the fields the resident arrays hold (body_view.h): a body is
// {pos, xVector, yVector, size} here (the reference's Geom keeps a copy of the frame, refreshed by UpdateGeom,
// RigidBody.h:38-42: the same values).  The functions are
// plain IEEE float arithmetic (no libm beyond fabsf, and the correctly rounded sqrtf of the round pairs) so the host loop and a HIP
// kernel that call them produce identical bits under -ffp-contract=off.  Round bodies (circle/circle, circle/box, the capsule pairs) have no counterpart
// in the reference: their rule is include/phyx_amd.h SHAPES; nor have convex polygons (include/phyx_amd.h POLYGONS).
#pragma once

#include "body_view.h"

namespace phx {

struct V2 { float x, y; };
__host__ __device__ __attribute__((always_inline)) inline V2 v2(float x, float y) { V2 r; r.x = x; r.y = y; return r; }
__host__ __device__ __attribute__((always_inline)) inline V2 v2(const phx_vec2& a) { return v2(a.x, a.y); }
__host__ __device__ __attribute__((always_inline)) inline V2 operator+(V2 a, V2 b) { return v2(a.x + b.x, a.y + b.y); }
__host__ __device__ __attribute__((always_inline)) inline V2 operator-(V2 a, V2 b) { return v2(a.x - b.x, a.y - b.y); }
__host__ __device__ __attribute__((always_inline)) inline V2 operator-(V2 a) { return v2(-a.x, -a.y); }
__host__ __device__ __attribute__((always_inline)) inline V2 operator*(V2 a, float s) { return v2(a.x * s, a.y * s); }
__host__ __device__ __attribute__((always_inline)) inline float dot(V2 a, V2 b) { return a.x * b.x + a.y * b.y; }           // ref: Vector2.h operator*(Vector2)
__host__ __device__ __attribute__((always_inline)) inline float sqlen(V2 a) { return a.x * a.x + a.y * a.y; }
__host__ __device__ __attribute__((always_inline)) inline V2 perp(V2 a) { return v2(-a.y, a.x); }                            // ref: Vector2.h GetPerpendicular
__host__ __device__ __attribute__((always_inline)) inline phx_vec2 pv(V2 a) { phx_vec2 r; r.x = a.x; r.y = a.y; return r; }

// what the narrowphase reads of a body (`kind`: PHX_SHAPE_BOX, PHX_SHAPE_CIRCLE or PHX_SHAPE_CAPSULE, include/phyx_amd.h SHAPES; a circle's radius
// is size.x, a capsule's size.y with the core segment size.x - size.y either way along xv)
// `poly`: the body's polygon record (PHX_SHAPE_POLYGON; include/phyx_amd.h POLYGONS), read by the polygon routines alone: null, and never
// looked at, in every instantiation without them
// (PolyRec: body_view.h)
struct NpBody { V2 pos, xv, yv, size; unsigned kind; const PolyRec* poly; };

// ref: Geom.h:79-85 RecomputeAABB: {min.x, min.y, max.x, max.y}
__host__ __device__ __attribute__((always_inline)) inline void geom_aabb(V2 pos, V2 xv, V2 yv, V2 size, float& minx, float& miny, float& maxx, float& maxy)
{
    const float dx = fabsf(xv.x) * size.x + fabsf(yv.x) * size.y;
    const float dy = fabsf(xv.y) * size.x + fabsf(yv.y) * size.y;
    minx = pos.x - dx; miny = pos.y - dy;
    maxx = pos.x + dx; maxy = pos.y + dy;
}

// ref: Geom.h:79-85 on a 128-byte record (uses the Geom copy of the frame, refreshed by UpdateGeom, RigidBody.h:38-42)
__host__ __device__ __attribute__((always_inline)) inline void update_geom(phx_rigid_body& b)
{
    b.geom_xvector = b.xvector; b.geom_yvector = b.yvector; b.geom_pos = b.pos;
    geom_aabb(v2(b.geom_pos), v2(b.geom_xvector), v2(b.geom_yvector), v2(b.geom_size), b.aabb_min.x, b.aabb_min.y, b.aabb_max.x, b.aabb_max.y);
}

// ref: Geom.h:66-77 with GetClippingEdge (:22-64) and GetClippingVertex (:10-20)
struct Support { V2 a, b; int n; };      // (returned by value: results written through references ended up behind a pointer phi, i.e. in scratch)
__host__ __device__ __attribute__((always_inline)) inline Support support_points(const NpBody& b, V2 axis)
{
    Support out;
    out.a = v2(0.f, 0.f); out.b = out.a;
    const V2 xv = b.xv, yv = b.yv, pos = b.pos;
    const V2 xdim = xv * b.size.x, ydim = yv * b.size.y;
    const float xdiff = dot(axis, xv), ydiff = dot(axis, yv);
    if (fabsf(xdiff) < 0.1f || fabsf(ydiff) < 0.1f) {
        V2 p1 = pos, p2 = pos, off = v2(0.f, 0.f);
        if (fabsf(xdiff) < fabsf(ydiff)) {
            if (dot(axis, ydim) > 0.0f) { off = off + ydim; p1 = p1 + xdim; p2 = p2 - xdim; }
            else                        { off = off - ydim; p1 = p1 - xdim; p2 = p2 + xdim; }
        } else {
            if (dot(axis, xdim) > 0.0f) { off = off + xdim; p1 = p1 - ydim; p2 = p2 + ydim; }
            else                        { off = off - xdim; p1 = p1 + ydim; p2 = p2 - ydim; }
        }
        out.a = p1 + off;
        out.b = p2 + off;
        out.n = 2;
        return out;
    }
    const float xs = dot(xv, axis) < 0.0f ? -1.0f : 1.0f;
    const float ys = dot(yv, axis) < 0.0f ? -1.0f : 1.0f;
    out.a = (pos + xdim * xs) + ydim * ys;
    out.n = 1;
    return out;
}

// ref: Collider.cpp:8-56 — returns false when a separating axis exists
__host__ __device__ __attribute__((always_inline)) inline bool least_penetration_axis(const NpBody& b1, const NpBody& b2, V2& axis)
{
    const V2 a00 = b1.xv, a01 = b1.yv, a10 = b2.xv, a11 = b2.yv;
    const V2 e0 = b1.size, e1 = b2.size;
    const V2 d = b1.pos - b2.pos;
    const float ad00 = fabsf(dot(a00, a10)), ad01 = fabsf(dot(a00, a11));
    const float r0 = e0.x + e1.x * ad00 + e1.y * ad01;
    const float d0 = fabsf(dot(a00, d)) - r0;
    if (d0 > 0) return false;
    float best = d0; V2 bestaxis = a00;
    const float ad10 = fabsf(dot(a01, a10)), ad11 = fabsf(dot(a01, a11));
    const float r1 = e0.y + e1.x * ad10 + e1.y * ad11;
    const float d1 = fabsf(dot(a01, d)) - r1;
    if (d1 > 0) return false;
    if (d1 > best) { best = d1; bestaxis = a01; }
    const float r2 = e1.x + e0.x * ad00 + e0.y * ad10;
    const float d2 = fabsf(dot(a10, d)) - r2;
    if (d2 > 0) return false;
    if (d2 > best) { best = d2; bestaxis = a10; }
    const float r3 = e1.y + e0.x * ad01 + e0.y * ad11;
    const float d3 = fabsf(dot(a11, d)) - r3;
    if (d3 > 0) return false;
    if (d3 > best) { best = d3; bestaxis = a11; }
    axis = bestaxis;
    return true;
}

// The manifold's working set of at most four contact points (two cached + two new, ref: Collider.cpp:215 newpoints[kMaxContactPoints * 2]).
// Four named members with static accessors instead of an array: an array indexed by a run-time count lives in scratch memory
// on the GPU (224 bytes per lane in round 2's kernel — a private-memory round trip for every point touched), members live in
// registers.
// (a contact point in registers: the record's four flag / padding bytes travel as one word — is_merged in bits 0-7,
//  is_newly_created in bits 8-15 — so that nothing is addressed byte-wise)
struct CpR { V2 d1, d2, n; unsigned flags; int si; };
__host__ __device__ __attribute__((always_inline)) inline CpR cp_load(const phx_contact_point& p)
{
    CpR r;
    r.d1 = v2(p.delta1); r.d2 = v2(p.delta2); r.n = v2(p.normal);
    r.flags = (unsigned)p.is_merged | ((unsigned)p.is_newly_created << 8) | ((unsigned)p.pad_[0] << 16) | ((unsigned)p.pad_[1] << 24);
    r.si = p.solver_index;
    return r;
}
__host__ __device__ __attribute__((always_inline)) inline void cp_store(phx_contact_point& p, const CpR& r)
{
    p.delta1 = pv(r.d1); p.delta2 = pv(r.d2); p.normal = pv(r.n);
    p.is_merged = (uint8_t)(r.flags & 0xFFu); p.is_newly_created = (uint8_t)((r.flags >> 8) & 0xFFu);
    p.pad_[0] = (uint8_t)((r.flags >> 16) & 0xFFu); p.pad_[1] = (uint8_t)(r.flags >> 24);
    p.solver_index = r.si;
}
struct Pts4 { CpR a, b, c, d; };
// (word by word: whole-struct copies under a run-time index keep the set in memory)
template <typename T> __host__ __device__ __attribute__((always_inline)) inline T sel4(int i, T a, T b, T c, T d) { return i == 0 ? a : (i == 1 ? b : (i == 2 ? c : d)); }
__host__ __device__ __attribute__((always_inline)) inline CpR pts_get(const Pts4& s, int i)
{
    CpR r;
    r.d1.x = sel4(i, s.a.d1.x, s.b.d1.x, s.c.d1.x, s.d.d1.x); r.d1.y = sel4(i, s.a.d1.y, s.b.d1.y, s.c.d1.y, s.d.d1.y);
    r.d2.x = sel4(i, s.a.d2.x, s.b.d2.x, s.c.d2.x, s.d.d2.x); r.d2.y = sel4(i, s.a.d2.y, s.b.d2.y, s.c.d2.y, s.d.d2.y);
    r.n.x = sel4(i, s.a.n.x, s.b.n.x, s.c.n.x, s.d.n.x); r.n.y = sel4(i, s.a.n.y, s.b.n.y, s.c.n.y, s.d.n.y);
    r.flags = sel4(i, s.a.flags, s.b.flags, s.c.flags, s.d.flags); r.si = sel4(i, s.a.si, s.b.si, s.c.si, s.d.si);
    return r;
}
__host__ __device__ __attribute__((always_inline)) inline void cp_put(CpR& dst, const CpR& v, bool on)
{
    dst.d1.x = on ? v.d1.x : dst.d1.x; dst.d1.y = on ? v.d1.y : dst.d1.y;
    dst.d2.x = on ? v.d2.x : dst.d2.x; dst.d2.y = on ? v.d2.y : dst.d2.y;
    dst.n.x = on ? v.n.x : dst.n.x; dst.n.y = on ? v.n.y : dst.n.y;
    dst.flags = on ? v.flags : dst.flags; dst.si = on ? v.si : dst.si;
}
__host__ __device__ __attribute__((always_inline)) inline void pts_set(Pts4& s, int i, const CpR& v)
{
    cp_put(s.a, v, i == 0); cp_put(s.b, v, i == 1); cp_put(s.c, v, i == 2); cp_put(s.d, v, i >= 3);
}

// ref: Collider.cpp:58-92 with ContactPoint::Equals (Manifold.h:31-38)
__host__ __device__ __attribute__((always_inline)) inline void merge_point(Pts4& pts, int& count, V2 p1, V2 p2, V2 n,
                                            const NpBody& b1, const NpBody& b2)
{
    const V2 d1 = p1 - b1.pos, d2 = p2 - b2.pos;                      // ref: Manifold.h:20-21
    int closest = -1;
    float bestdepth = 3.402823466e+38f;
    auto consider = [&](const CpR& q, int i) {                        // the reference's loop over the points, in index order
        if (i >= count) return;
        const float s1 = sqlen(q.d1 - d1), s2 = sqlen(q.d2 - d2);
        if (s1 > 2.0f * 2.0f && s2 > 2.0f * 2.0f) return;             // !Equals(col, 2.0f)
        const float depth = sqlen(d1 - q.d1) + sqlen(d2 - q.d2);
        if (depth < bestdepth) { bestdepth = depth; closest = i; }
    };
    consider(pts.a, 0); consider(pts.b, 1); consider(pts.c, 2); consider(pts.d, 3);
    if (closest >= 0) {
        CpR c = pts_get(pts, closest);
        c.flags = (c.flags & 0xFFFF0000u) | 1u;                        // isMerged = true, isNewlyCreated = false
        c.n = n; c.d1 = d1; c.d2 = d2;
        pts_set(pts, closest, c);
    } else {
        CpR c;
        c.d1 = d1; c.d2 = d2; c.n = n;
        c.flags = 1u | (1u << 8);                                      // merged, newly created
        c.si = -1;
        pts_set(pts, count, c);
        ++count;
    }
}

// ref: Vector2.h ProjectPointToLine(point, planePoint, planeNormal, projectionDirection, out)
__host__ __device__ __attribute__((always_inline)) inline V2 project_to_line(V2 point, V2 plane_point, V2 plane_normal, V2 dir)
{
    const float mult = 1.0f / dot(dir, plane_normal);
    const float s = dot(plane_point, plane_normal) - dot(point, plane_normal);
    return point + (dir * s) * mult;
}

__host__ __device__ __attribute__((always_inline)) inline bool within_segment(V2 p, V2 a, V2 b)
{
    return dot(p - a, b - a) >= 0.0f && dot(p - b, a - b) >= 0.0f;
}

// ref: Collider.cpp:94-209
__host__ __device__ __attribute__((always_inline)) inline void generate_contacts(const NpBody& b1, const NpBody& b2, Pts4& pts, int& count, V2 axis)
{
    if (dot(axis, b1.pos - b2.pos) < 0.0f) axis = -axis;
    const Support sp1 = support_points(b1, -axis), sp2 = support_points(b2, axis);
    V2 s10 = sp1.a, s11 = sp1.b, s20 = sp2.a, s21 = sp2.b;          // (named, not indexed: see Pts4)
    int n1 = sp1.n, n2 = sp2.n;
    const float tol = 2.0f;
    if (n1 == 2 && sqlen(s10 - s11) < tol * tol) { s10 = (s10 + s11) * 0.5f; n1 = 1; }
    if (n2 == 2 && sqlen(s20 - s21) < tol * tol) { s20 = (s20 + s21) * 0.5f; n2 = 1; }

    if (n1 == 1 && n2 == 1) {
        if (dot(s20 - s10, axis) >= 0.0f) merge_point(pts, count, s10, s20, axis, b1, b2);
    } else if (n1 == 1 && n2 == 2) {
        const V2 p = project_to_line(s10, s20, perp(s21 - s20), axis);
        if (within_segment(p, s20, s21)) merge_point(pts, count, s10, p, axis, b1, b2);
    } else if (n1 == 2 && n2 == 1) {
        const V2 p = project_to_line(s20, s10, perp(s11 - s10), axis);
        if (within_segment(p, s10, s11)) merge_point(pts, count, p, s20, axis, b1, b2);
    } else {
        // up to four candidate pairs in the reference's tempCol[4] (ref: Collider.cpp:160-200); only the first two found are ever
        // merged, so only those two are kept (named, not indexed: see Pts4)
        // the four candidates in the reference's order, each with its 'found' flag; the first two found are picked by selects
        const V2 nrm2 = perp(s21 - s20), nrm1 = perp(s11 - s10);
        const V2 p0 = project_to_line(s10, s20, nrm2, axis), p1 = project_to_line(s11, s20, nrm2, axis);
        const V2 p2 = project_to_line(s20, s10, nrm1, axis), p3 = project_to_line(s21, s10, nrm1, axis);
        const bool f0 = dot(s10 - s20, nrm2) >= 0.0f && within_segment(p0, s20, s21);
        const bool f1 = dot(s11 - s20, nrm2) >= 0.0f && within_segment(p1, s20, s21);
        const bool f2 = dot(s20 - s10, nrm1) >= 0.0f && within_segment(p2, s10, s11);
        const bool f3 = dot(s21 - s10, nrm1) >= 0.0f && within_segment(p3, s10, s11);
        const int tc = (f0 ? 1 : 0) + (f1 ? 1 : 0) + (f2 ? 1 : 0) + (f3 ? 1 : 0);
        const int k0 = f0 ? 0 : (f1 ? 1 : (f2 ? 2 : 3));                                   // first found
        const int k1 = k0 == 0 ? (f1 ? 1 : (f2 ? 2 : 3)) : (k0 == 1 ? (f2 ? 2 : 3) : 3);   // second found (if there is one)
        // candidate k = (point on body 1, point on body 2): {s10, p0}, {s11, p1}, {p2, s20}, {p3, s21}
        const V2 ta0 = v2(sel4(k0, s10.x, s11.x, p2.x, p3.x), sel4(k0, s10.y, s11.y, p2.y, p3.y));
        const V2 tb0 = v2(sel4(k0, p0.x, p1.x, s20.x, s21.x), sel4(k0, p0.y, p1.y, s20.y, s21.y));
        const V2 ta1 = v2(sel4(k1, s10.x, s11.x, p2.x, p3.x), sel4(k1, s10.y, s11.y, p2.y, p3.y));
        const V2 tb1 = v2(sel4(k1, p0.x, p1.x, s20.x, s21.x), sel4(k1, p0.y, p1.y, s20.y, s21.y));
        if (tc == 1) merge_point(pts, count, ta0, tb0, axis, b1, b2);
        if (tc >= 2) {
            merge_point(pts, count, ta0, tb0, axis, b1, b2);
            merge_point(pts, count, ta1, tb1, axis, b1, b2);
        }
    }
}

// ---- round bodies (include/phyx_amd.h SHAPES; tests/circle_spec.py states the two routines as the same expressions) ----------------
// Both feed merge_point with at most one point; the normal points from body2 towards body1 and (p2 - p1) . n >= 0 is the penetration,
// as for boxes.  Every operation is rounded on its own; sqrtf and / are correctly rounded under the library's flags (pin_kernels.h).
__host__ __device__ __attribute__((always_inline)) inline void circle_circle_contact(const NpBody& b1, const NpBody& b2, Pts4& pts, int& count)
{
    const float r1 = b1.size.x, r2 = b2.size.x;
    const V2 d = b1.pos - b2.pos;
    const float l2 = dot(d, d), R = r1 + r2;
    if (l2 > R * R) return;
    const float l = sqrtf(l2);
    const V2 n = l > 0.0f ? v2(d.x / l, d.y / l) : v2(1.0f, 0.0f);
    merge_point(pts, count, b1.pos - n * r1, b2.pos + n * r2, n, b1, b2);
}

// circle `c` against box `b`; `circle_first`: the circle is the manifold's body1
__host__ __device__ __attribute__((always_inline)) inline void circle_box_contact(const NpBody& c, const NpBody& b, bool circle_first, Pts4& pts, int& count,
                                                                                  const NpBody& b1, const NpBody& b2)
{
    const V2 xv = b.xv, yv = b.yv, h = b.size;
    const float r = c.size.x;
    const V2 rel = c.pos - b.pos;
    const float u = dot(rel, xv), v = dot(rel, yv);
    float qu = u < -h.x ? -h.x : (u > h.x ? h.x : u);
    float qv = v < -h.y ? -h.y : (v > h.y ? h.y : v);
    V2 N;
    if (qu == u && qv == v) {                                           // the centre is inside or on the box: the face of least depth
        const float pu = h.x - fabsf(u), pv_ = h.y - fabsf(v);
        if (pu <= pv_) { N = u < 0.0f ? -xv : xv; qu = u < 0.0f ? -h.x : h.x; }
        else           { N = v < 0.0f ? -yv : yv; qv = v < 0.0f ? -h.y : h.y; }
    } else {
        const V2 e = v2(u - qu, v - qv);
        const float l2 = dot(e, e);
        if (l2 > r * r) return;
        const float l = sqrtf(l2);
        N = xv * (e.x / l) + yv * (e.y / l);
    }
    const V2 on_box = (b.pos + xv * qu) + yv * qv;
    const V2 on_circle = c.pos - N * r;
    if (circle_first) merge_point(pts, count, on_circle, on_box, N, b1, b2);
    else              merge_point(pts, count, on_box, on_circle, -N, b1, b2);
}

// ---- capsules (include/phyx_amd.h SHAPES; tests/capsule_spec.py states what follows as the same expressions) -----------------------
// A capsule is the segment pos -+ xv*a, a = size.x - size.y, with the radius r = size.y.  A pair with a capsule yields up to six
// candidates, each a disc (an end of a capsule, a circle, a box's corner as a disc of radius 0) against the other shape, and up to two
// of them are merged.  A candidate is kept in the manifold's order: p1 on body1, p2 on body2, n from body2 towards body1.
struct Cand { V2 p1, p2, n; float depth; bool ok; };
__host__ __device__ __attribute__((always_inline)) inline Cand cand_none()
{
    Cand c;
    c.p1 = c.p2 = c.n = v2(0.f, 0.f); c.depth = 0.f; c.ok = false;
    return c;
}
// `disc_first`: the disc belongs to body1; N points from the other shape towards the disc
__host__ __device__ __attribute__((always_inline)) inline Cand cand_make(V2 on_disc, V2 on_other, V2 N, float depth, bool disc_first)
{
    Cand c;
    c.p1 = disc_first ? on_disc : on_other; c.p2 = disc_first ? on_other : on_disc; c.n = disc_first ? N : -N;
    c.depth = depth; c.ok = true;
    return c;
}
__host__ __device__ __attribute__((always_inline)) inline float capsule_half(const NpBody& k) { return k.size.x - k.size.y; }

// the disc {cpos, r} against box b: circle_box_contact's arithmetic, with the depth
__host__ __device__ __attribute__((always_inline)) inline Cand disc_box_cand(V2 cpos, float r, const NpBody& b, bool disc_first)
{
    const V2 xv = b.xv, yv = b.yv, h = b.size;
    const V2 rel = cpos - b.pos;
    const float u = dot(rel, xv), v = dot(rel, yv);
    float qu = u < -h.x ? -h.x : (u > h.x ? h.x : u);
    float qv = v < -h.y ? -h.y : (v > h.y ? h.y : v);
    V2 N;
    float depth;
    if (qu == u && qv == v) {
        const float pu = h.x - fabsf(u), pv_ = h.y - fabsf(v);
        if (pu <= pv_) { N = u < 0.0f ? -xv : xv; qu = u < 0.0f ? -h.x : h.x; depth = r + pu; }
        else           { N = v < 0.0f ? -yv : yv; qv = v < 0.0f ? -h.y : h.y; depth = r + pv_; }
    } else {
        const V2 e = v2(u - qu, v - qv);
        const float l2 = dot(e, e);
        if (l2 > r * r) return cand_none();
        const float l = sqrtf(l2);
        N = xv * (e.x / l) + yv * (e.y / l);
        depth = r - l;
    }
    const V2 on_box = (b.pos + xv * qu) + yv * qv;
    return cand_make(cpos - N * r, on_box, N, depth, disc_first);
}

// the disc {c, rc} against capsule k; `unclamped`: the nearest point of the core segment is not an end (qu == u)
__host__ __device__ __attribute__((always_inline)) inline Cand disc_capsule_cand(V2 c, float rc, const NpBody& k, bool disc_first, bool& unclamped)
{
    const V2 xv = k.xv, yv = k.yv;
    const float r = k.size.y, a = capsule_half(k);
    const V2 e = c - k.pos;
    const float u = dot(e, xv), v = dot(e, yv);
    const float qu = u < -a ? -a : (u > a ? a : u);
    const V2 g = v2(u - qu, v);
    const float l2 = dot(g, g), R = r + rc;
    unclamped = qu == u;
    if (l2 > R * R) return cand_none();
    const float l = sqrtf(l2);
    const V2 N = l > 0.0f ? xv * (g.x / l) + yv * (g.y / l) : yv;
    const V2 on_capsule = (k.pos + xv * qu) + N * r;
    return cand_make(c - N * rc, on_capsule, N, R - l, disc_first);
}

// The selection: the first point is the deepest candidate (the first in order on a tie); the second is, among the others that are
// distinct from the first under ContactPoint::Equals(2.0f) (both points more than 2 apart), the one whose p1 is farthest from the
// first's (the first in order on a tie).  A running best over named candidates: no array under a run-time index (Pts4).
__host__ __device__ __attribute__((always_inline)) inline void capsule_select(const Cand& c0, const Cand& c1, const Cand& c2, const Cand& c3, const Cand& c4,
                                                                              const Cand& c5, Pts4& pts, int& count, const NpBody& b1, const NpBody& b2)
{
    Cand first = cand_none();
    int fi = -1;
    auto deeper = [&](const Cand& c, int i) { if (c.ok && (fi < 0 || c.depth > first.depth)) { first = c; fi = i; } };
    deeper(c0, 0); deeper(c1, 1); deeper(c2, 2); deeper(c3, 3); deeper(c4, 4); deeper(c5, 5);
    if (fi < 0) return;
    Cand second = cand_none();
    int si = -1;
    float sep = 0.0f;
    auto farther = [&](const Cand& c, int i) {
        if (!c.ok || i == fi) return;
        const float s1 = sqlen(c.p1 - first.p1), s2 = sqlen(c.p2 - first.p2);
        if (!(s1 > 2.0f * 2.0f && s2 > 2.0f * 2.0f)) return;
        if (si < 0 || s1 > sep) { second = c; sep = s1; si = i; }
    };
    farther(c0, 0); farther(c1, 1); farther(c2, 2); farther(c3, 3); farther(c4, 4); farther(c5, 5);
    merge_point(pts, count, first.p1, first.p2, first.n, b1, b2);
    if (si >= 0) merge_point(pts, count, second.p1, second.p2, second.n, b1, b2);
}

// a pair with a capsule (`b1`, `b2` in the manifold's order)
__host__ __device__ __attribute__((always_inline)) inline void capsule_contact(const NpBody& b1, const NpBody& b2, Pts4& pts, int& count)
{
    const unsigned CAPSULE = (unsigned)PHX_SHAPE_CAPSULE, CIRCLE = (unsigned)PHX_SHAPE_CIRCLE;
    Cand c0 = cand_none(), c1 = c0, c2 = c0, c3 = c0, c4 = c0, c5 = c0;
    bool free_ = false;
    if (b1.kind == CAPSULE && b2.kind == CAPSULE) {                     // A's ends against B, then B's ends against A where they meet its side
        const float a1 = capsule_half(b1), a2 = capsule_half(b2);
        c0 = disc_capsule_cand(b1.pos - b1.xv * a1, b1.size.y, b2, true, free_);
        c1 = disc_capsule_cand(b1.pos + b1.xv * a1, b1.size.y, b2, true, free_);
        c2 = disc_capsule_cand(b2.pos - b2.xv * a2, b2.size.y, b1, false, free_); c2.ok = c2.ok && free_;
        c3 = disc_capsule_cand(b2.pos + b2.xv * a2, b2.size.y, b1, false, free_); c3.ok = c3.ok && free_;
    } else if (b1.kind == CIRCLE || b2.kind == CIRCLE) {                // the circle's disc against the capsule
        const bool circle_first = b1.kind == CIRCLE;
        const NpBody& c = circle_first ? b1 : b2;
        const NpBody& k = circle_first ? b2 : b1;
        c0 = disc_capsule_cand(c.pos, c.size.x, k, circle_first, free_);
    } else {                                                            // the capsule's ends against the box, then the box's corners against the capsule's side
        const bool capsule_first = b1.kind == CAPSULE;
        const NpBody& k = capsule_first ? b1 : b2;
        const NpBody& b = capsule_first ? b2 : b1;
        const float a = capsule_half(k);
        const V2 h = b.size;
        c0 = disc_box_cand(k.pos - k.xv * a, k.size.y, b, capsule_first);
        c1 = disc_box_cand(k.pos + k.xv * a, k.size.y, b, capsule_first);
        c2 = disc_capsule_cand((b.pos + b.xv * -h.x) + b.yv * -h.y, 0.0f, k, !capsule_first, free_); c2.ok = c2.ok && free_;
        c3 = disc_capsule_cand((b.pos + b.xv * h.x) + b.yv * -h.y, 0.0f, k, !capsule_first, free_); c3.ok = c3.ok && free_;
        c4 = disc_capsule_cand((b.pos + b.xv * -h.x) + b.yv * h.y, 0.0f, k, !capsule_first, free_); c4.ok = c4.ok && free_;
        c5 = disc_capsule_cand((b.pos + b.xv * h.x) + b.yv * h.y, 0.0f, k, !capsule_first, free_); c5.ok = c5.ok && free_;
    }
    capsule_select(c0, c1, c2, c3, c4, c5, pts, count, b1, b2);
}

// ---- convex polygons (include/phyx_amd.h POLYGONS; tests/polygon_spec.py is the definition and states what follows as the same expressions) ----
// The stored record of a polygon: the vertices and n_k, the unit outward normal of the edge v_k -> v_(k+1): e = v_next - v_k,
// l = sqrtf(dot(e, e)), n = (e.y / l, -e.x / l).  One function for the host path and the device path: the same bytes.
__host__ __device__ inline PolyRec poly_record(const phx_polygon& p)
{
    PolyRec r;
    r.count = p.count;
    for (int k = 0; k < PHX_POLYGON_MAX_VERTICES; ++k) { r.v[2 * k] = 0.f; r.v[2 * k + 1] = 0.f; r.n[2 * k] = 0.f; r.n[2 * k + 1] = 0.f; }
    const int c = p.count < 0 ? 0 : (p.count > PHX_POLYGON_MAX_VERTICES ? PHX_POLYGON_MAX_VERTICES : p.count);
    for (int k = 0; k < c; ++k) {
        const int k1 = k + 1 < c ? k + 1 : 0;
        const V2 a = v2(p.v[k]), e = v2(p.v[k1]) - a;
        const float l = sqrtf(dot(e, e));
        r.v[2 * k] = a.x; r.v[2 * k + 1] = a.y;
        r.n[2 * k] = e.y / l; r.n[2 * k + 1] = -e.x / l;
    }
    return r;
}

// In a pair with a polygon a box is the 4-gon (-hx,-hy), (hx,-hy), (hx,hy), (-hx,hy) with the exact normals (0,-1), (1,0), (0,1), (-1,0).
// Vertices and normals are read through the record's pointer (memory under a run-time index) or formed by selects: no private array.
__host__ __device__ __attribute__((always_inline)) inline bool is_polygon(const NpBody& b) { return b.kind == (unsigned)PHX_SHAPE_POLYGON; }
__host__ __device__ __attribute__((always_inline)) inline int poly_count(const NpBody& b) { return is_polygon(b) ? b.poly->count : 4; }
__host__ __device__ __attribute__((always_inline)) inline V2 poly_v(const NpBody& b, int k)
{
    if (is_polygon(b)) return v2(b.poly->v[2 * k], b.poly->v[2 * k + 1]);
    return v2((k == 1 || k == 2) ? b.size.x : -b.size.x, k >= 2 ? b.size.y : -b.size.y);
}
__host__ __device__ __attribute__((always_inline)) inline V2 poly_n(const NpBody& b, int k)
{
    if (is_polygon(b)) return v2(b.poly->n[2 * k], b.poly->n[2 * k + 1]);
    return v2(k == 1 ? 1.0f : (k == 3 ? -1.0f : 0.0f), k == 0 ? -1.0f : (k == 2 ? 1.0f : 0.0f));
}
__host__ __device__ __attribute__((always_inline)) inline V2 poly_wv(const NpBody& b, int k) { const V2 v = poly_v(b, k); return (b.pos + b.xv * v.x) + b.yv * v.y; }
__host__ __device__ __attribute__((always_inline)) inline V2 poly_wn(const NpBody& b, int k) { const V2 n = poly_n(b, k); return b.xv * n.x + b.yv * n.y; }

// one of two bodies by value, member by member: a reference chosen at run time and read inside a loop is a pointer into private memory,
// which puts both bodies in scratch (Support, above)
__host__ __device__ __attribute__((always_inline)) inline NpBody np_pick(bool first, const NpBody& a, const NpBody& b)
{
    NpBody r;
    r.pos = v2(first ? a.pos.x : b.pos.x, first ? a.pos.y : b.pos.y); r.xv = v2(first ? a.xv.x : b.xv.x, first ? a.xv.y : b.xv.y);
    r.yv = v2(first ? a.yv.x : b.yv.x, first ? a.yv.y : b.yv.y); r.size = v2(first ? a.size.x : b.size.x, first ? a.size.y : b.size.y);
    r.kind = first ? a.kind : b.kind; r.poly = first ? a.poly : b.poly;
    return r;
}

// the face of `a` of largest separation from `b`: s_i = min_j dot(NA_i, wB_j - wA_i), the largest s_i, the first on a tie
struct FaceSep { float s; int i; };
__host__ __device__ __attribute__((always_inline)) inline FaceSep poly_face_sep(const NpBody& a, const NpBody& b)
{
    FaceSep out;
    out.s = 0.f; out.i = 0;
    const int na = poly_count(a), nb = poly_count(b);
    for (int i = 0; i < na; ++i) {
        const V2 w = poly_wv(a, i), N = poly_wn(a, i);
        float s = dot(N, poly_wv(b, 0) - w);
        for (int j = 1; j < nb; ++j) { const float d = dot(N, poly_wv(b, j) - w); if (d < s) s = d; }
        if (i == 0 || s > out.s) { out.s = s; out.i = i; }
    }
    return out;
}

// one side plane: the segment p0 p1 cut to d >= 0; false when nothing is left
__host__ __device__ __attribute__((always_inline)) inline bool poly_clip(V2& p0, V2& p1, float d0, float d1)
{
    if (d0 < 0.0f && d1 < 0.0f) return false;
    if (d0 < 0.0f) p0 = p0 + (p1 - p0) * (d0 / (d0 - d1));
    else if (d1 < 0.0f) p1 = p1 + (p0 - p1) * (d1 / (d1 - d0));
    return true;
}

// polygon / polygon and polygon / box (`b1`, `b2` in the manifold's order)
__host__ __device__ __attribute__((always_inline)) inline void polygon_polygon_contact(const NpBody& b1, const NpBody& b2, Pts4& pts, int& count)
{
    const FaceSep fa = poly_face_sep(b1, b2);
    if (fa.s > 0.0f) return;
    const FaceSep fb = poly_face_sep(b2, b1);
    if (fb.s > 0.0f) return;
    const bool ref_first = !(fb.s > fa.s);
    const NpBody R = np_pick(ref_first, b1, b2), I = np_pick(ref_first, b2, b1);
    const int ri = ref_first ? fa.i : fb.i, nr = poly_count(R), ni = poly_count(I);
    const V2 r0 = poly_wv(R, ri), r1 = poly_wv(R, ri + 1 < nr ? ri + 1 : 0), Nr = poly_wn(R, ri);
    int inc = 0;
    float least = dot(Nr, poly_wn(I, 0));
    for (int j = 1; j < ni; ++j) { const float d = dot(Nr, poly_wn(I, j)); if (d < least) { least = d; inc = j; } }
    V2 p0 = poly_wv(I, inc), p1 = poly_wv(I, inc + 1 < ni ? inc + 1 : 0);
    const V2 e = r1 - r0;
    if (!poly_clip(p0, p1, dot(p0 - r0, e), dot(p1 - r0, e))) return;
    if (!poly_clip(p0, p1, dot(r1 - p0, e), dot(r1 - p1, e))) return;
    const float s0 = dot(Nr, p0 - r0), s1 = dot(Nr, p1 - r0);
    if (s0 <= 0.0f) { if (ref_first) merge_point(pts, count, p0 - Nr * s0, p0, -Nr, b1, b2); else merge_point(pts, count, p0, p0 - Nr * s0, Nr, b1, b2); }
    if (s1 <= 0.0f) { if (ref_first) merge_point(pts, count, p1 - Nr * s1, p1, -Nr, b1, b2); else merge_point(pts, count, p1, p1 - Nr * s1, Nr, b1, b2); }
}

// the disc {c, r} against polygon (or 4-gon box) P: the building block, as disc_box_cand is for boxes
__host__ __device__ __attribute__((always_inline)) inline Cand disc_polygon_cand(V2 c, float r, const NpBody& P, bool disc_first)
{
    const V2 g = c - P.pos;
    const V2 p = v2(dot(g, P.xv), dot(g, P.yv));
    const int n = poly_count(P);
    int k = 0;
    float s = dot(poly_n(P, 0), p - poly_v(P, 0));
    for (int j = 1; j < n; ++j) { const float d = dot(poly_n(P, j), p - poly_v(P, j)); if (d > s) { s = d; k = j; } }
    if (s > r) return cand_none();
    const V2 vk = poly_v(P, k), nk = poly_n(P, k);
    V2 Nl = nk, q = p - nk * s;
    float depth = r - s;
    if (s > 0.0f) {
        const V2 vn = poly_v(P, k + 1 < n ? k + 1 : 0);
        const V2 e = vn - vk;
        const float t = dot(p - vk, e);
        const bool lo = t < 0.0f, hi = !lo && t > dot(e, e);
        if (lo || hi) {
            q = lo ? vk : vn;
            const V2 h = p - q;
            const float l2 = dot(h, h);
            if (l2 > r * r) return cand_none();
            const float l = sqrtf(l2);
            Nl = v2(h.x / l, h.y / l);
            depth = r - l;
        }
    }
    const V2 N = P.xv * Nl.x + P.yv * Nl.y;
    const V2 on_poly = (P.pos + P.xv * q.x) + P.yv * q.y;
    return cand_make(c - N * r, on_poly, N, depth, disc_first);
}

// capsule K against polygon P: candidate i of the stream: 0, 1 K's end discs against P; 2 + k P's vertex k as a disc of radius 0
// against K, only if unclamped
__host__ __device__ __attribute__((always_inline)) inline Cand capsule_polygon_cand(const NpBody& K, const NpBody& P, bool capsule_first, int i)
{
    if (i < 2) {
        const float a = capsule_half(K);
        return disc_polygon_cand(i == 0 ? K.pos - K.xv * a : K.pos + K.xv * a, K.size.y, P, capsule_first);
    }
    bool free_ = false;
    Cand c = disc_capsule_cand(poly_wv(P, i - 2), 0.0f, K, !capsule_first, free_);
    c.ok = c.ok && free_;
    return c;
}

// capsule_select's rule, word for word, as a running selection over a stream of `n` candidates gen(i): the stream is walked twice and
// nothing is kept but the two bests, in named registers
template <class Gen>
__host__ __device__ __attribute__((always_inline)) inline void select_stream(Gen gen, int n, Pts4& pts, int& count, const NpBody& b1, const NpBody& b2)
{
    Cand first = cand_none();
    int fi = -1;
    for (int i = 0; i < n; ++i) { const Cand c = gen(i); if (c.ok && (fi < 0 || c.depth > first.depth)) { first = c; fi = i; } }
    if (fi < 0) return;
    Cand second = cand_none();
    int si = -1;
    float sep = 0.0f;
    for (int i = 0; i < n; ++i) {
        if (i == fi) continue;
        const Cand c = gen(i);
        if (!c.ok) continue;
        const float s1 = sqlen(c.p1 - first.p1), s2 = sqlen(c.p2 - first.p2);
        if (!(s1 > 2.0f * 2.0f && s2 > 2.0f * 2.0f)) continue;
        if (si < 0 || s1 > sep) { second = c; sep = s1; si = i; }
    }
    merge_point(pts, count, first.p1, first.p2, first.n, b1, b2);
    if (si >= 0) merge_point(pts, count, second.p1, second.p2, second.n, b1, b2);
}

// a pair with a polygon (`b1`, `b2` in the manifold's order)
__host__ __device__ __attribute__((always_inline)) inline void polygon_contact(const NpBody& b1, const NpBody& b2, Pts4& pts, int& count)
{
    const unsigned CAPSULE = (unsigned)PHX_SHAPE_CAPSULE, CIRCLE = (unsigned)PHX_SHAPE_CIRCLE;
    const bool poly_first = is_polygon(b1);
    const NpBody P = np_pick(poly_first, b1, b2), O = np_pick(poly_first, b2, b1);      // (the other body: any kind; a polygon only when both are)
    if (O.kind == CIRCLE) {
        const Cand c = disc_polygon_cand(O.pos, O.size.x, P, !poly_first);
        if (c.ok) merge_point(pts, count, c.p1, c.p2, c.n, b1, b2);
    } else if (O.kind == CAPSULE) {
        select_stream([&](int i) { return capsule_polygon_cand(O, P, !poly_first, i); }, 2 + poly_count(P), pts, count, b1, b2);
    } else polygon_polygon_contact(b1, b2, pts, count);
}

// ref: Collider.cpp:211-245.  Returns true if a third merged point had to be dropped: the reference
// would write it past the manifold's two slots (only an assert guards it).
// The pair's kinds pick the routine in front of least_penetration_axis; a caller whose kinds are the constant PHX_SHAPE_BOX (a world
// without a shape column) compiles to the box/box code alone.  CAPSULES: a kind may be PHX_SHAPE_CAPSULE (a world that made one);
// without it every kind that is not a box is a circle and the capsule routines are not compiled in.  POLYGONS: a kind may be
// PHX_SHAPE_POLYGON (a world that made one); a pair with one takes polygon_contact, every other pair the code above, unchanged.
template <bool CAPSULES = false, bool POLYGONS = false>
__host__ __device__ __attribute__((always_inline)) inline bool update_manifold(phx_manifold& m, const NpBody& b1, const NpBody& b2, phx_contact_point* pts)
{
    Pts4 np;
    CpR blank;
    blank.d1 = blank.d2 = blank.n = v2(0.f, 0.f); blank.flags = 0u; blank.si = -1;
    np.a = np.b = np.c = np.d = blank;                                  // (slots at and beyond `count` are never looked at)
    if (m.point_count > 0) { np.a = cp_load(pts[0]); np.a.flags &= 0xFFFF0000u; }      // isMerged = isNewlyCreated = false
    if (m.point_count > 1) { np.b = cp_load(pts[1]); np.b.flags &= 0xFFFF0000u; }
    int count = m.point_count;
    if (POLYGONS && (is_polygon(b1) || is_polygon(b2))) polygon_contact(b1, b2, np, count);
    else if ((b1.kind | b2.kind) == 0u) {
        V2 axis;
        if (least_penetration_axis(b1, b2, axis)) generate_contacts(b1, b2, np, count, axis);
    } else if (CAPSULES && (b1.kind == (unsigned)PHX_SHAPE_CAPSULE || b2.kind == (unsigned)PHX_SHAPE_CAPSULE)) capsule_contact(b1, b2, np, count);
    else if (b1.kind != 0u && b2.kind != 0u) circle_circle_contact(b1, b2, np, count);
    else if (b1.kind != 0u) circle_box_contact(b1, b2, true, np, count, b1, b2);
    else circle_box_contact(b2, b1, false, np, count, b1, b2);
    m.point_count = 0;
    bool dropped = false;
    auto keep = [&](const CpR& q, int i) {
        if (i >= count || !(q.flags & 0xFFu)) return;
        if (m.point_count < 2) cp_store(pts[m.point_count++], q);
        else dropped = true;
    };
    keep(np.a, 0); keep(np.b, 1); keep(np.c, 2); keep(np.d, 3);
    return dropped;
}

// ref: AABB2.h:19-24 on {min.x, min.y, max.x, max.y}
__host__ __device__ __attribute__((always_inline)) inline bool aabb_intersects(const float4& a, const float4& b)
{
    if (a.x > b.z || b.x > a.z) return false;
    if (a.y > b.w || b.y > a.w) return false;
    return true;
}

} // namespace phx
