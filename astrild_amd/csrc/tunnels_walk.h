// The walk of the tunnels void finder (tunnels.hip): the star of one tracer, by gift wrapping over a uniform 2D cell
// grid, done by one wave whose lanes scan candidate tracers in parallel and reduce across the wave.  Every decision is
// exact integer arithmetic (coordinate differences below 2^14 keep the in-circle determinant below 2^60).
//
// The text is written against TN_WAVE lanes, TN_SHFL_XOR and TN_ATOMIC_ADD, which tunnels.hip defines as 64,
// __shfl_xor and atomicAdd.  Every shuffle sits in control flow that the whole wave executes, so with host threads as
// lanes and shuffles through a shared array between barriers the same text runs on a CPU, which is how the walk's
// logic can be exercised without a GPU.
#pragma once

namespace tn {

typedef long long i64;
typedef unsigned long long u64;

struct Pt { int x, y; };
struct Obj { int x, y; unsigned id, pad; };     // a tracer: pixel coordinates and its index in the caller's arrays

// Cells of cs x cs pixels, gdim per axis, cell (cx, cy) = cy * gdim + cx; pts sorted by cell, cell c holds
// pts[cell_start[c] .. cell_start[c + 1]).  A row of cells is therefore one contiguous range of pts.
struct Grid {
    int npix, cs, gdim;
    unsigned n;
    const Obj* pts;
    const unsigned* cell_start;
};

struct Out {
    i64* records;                               // [cap][7]: i, e, k, n_on, X, Y, W
    u64* count;                                 // [0] records appended, [1] violations
    u64 cap;
};

struct Box { int x0, y0, x1, y1; };             // cells, inclusive; x0 > x1: empty

// > 0: c strictly left of a -> b.
TN_DEV inline i64 orient(Pt a, Pt b, Pt c) {
    return (i64)(b.x - a.x) * (c.y - a.y) - (i64)(b.y - a.y) * (c.x - a.x);
}

// (a, b, c) counter-clockwise; > 0: d strictly inside their circle, 0: on it.
TN_DEV inline i64 incircle(Pt a, Pt b, Pt c, Pt d) {
    const i64 ax = a.x - d.x, ay = a.y - d.y, bx = b.x - d.x, by = b.y - d.y, cx = c.x - d.x, cy = c.y - d.y;
    return (ax * ax + ay * ay) * (bx * cy - by * cx) - (bx * bx + by * by) * (ax * cy - ay * cx) +
           (cx * cx + cy * cy) * (ax * by - ay * bx);
}

TN_DEV inline i64 floor_div(i64 n, i64 d) {     // d > 0
    i64 q = n / d;
    if (n % d != 0 && n < 0) --q;
    return q;
}

// The circle of the counter-clockwise triple (a, b, c): centre (X / W, Y / W), W = 2 D > 0; (Ux, Uy) / W = centre - a.
TN_DEV inline void circle(Pt a, Pt b, Pt c, i64& X, i64& Y, i64& W, i64& Ux, i64& Uy) {
    const i64 bx = b.x - a.x, by = b.y - a.y, cx = c.x - a.x, cy = c.y - a.y;
    const i64 b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
    W = 2 * (bx * cy - by * cx);
    Ux = cy * b2 - by * c2;
    Uy = bx * c2 - cx * b2;
    X = W * a.x + Ux;
    Y = W * a.y + Uy;
}

TN_DEV inline int clampi(i64 v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// Cells under the bounding box of the circle of (a, b, c), clipped to the map.  The radius times W is bounded from
// above by max(|Ux|, |Uy|) + ceil(min(|Ux|, |Uy|) / 2) >= hypot(Ux, Uy), so no square root is taken.  The circle
// passes through a, which lies in the map, so the clipped box is never empty.
TN_DEV inline Box circle_box(const Grid& g, Pt a, Pt b, Pt c) {
    i64 X, Y, W, Ux, Uy;
    circle(a, b, c, X, Y, W, Ux, Uy);
    const i64 ux = Ux < 0 ? -Ux : Ux, uy = Uy < 0 ? -Uy : Uy;
    const i64 R = (ux > uy ? ux : uy) + ((ux > uy ? uy : ux) + 1) / 2;
    const int top = g.npix - 1;
    Box o;
    o.x0 = clampi(floor_div(X - R, W), 0, top) / g.cs;
    o.x1 = clampi(floor_div(X + R, W) + 1, 0, top) / g.cs;
    o.y0 = clampi(floor_div(Y - R, W), 0, top) / g.cs;
    o.y1 = clampi(floor_div(Y + R, W) + 1, 0, top) / g.cs;
    return o;
}

TN_DEV inline Box clip_box(const Grid& g, int x0, int y0, int x1, int y1) {
    Box o;
    o.x0 = x0 < 0 ? 0 : x0;
    o.y0 = y0 < 0 ? 0 : y0;
    o.x1 = x1 > g.gdim - 1 ? g.gdim - 1 : x1;
    o.y1 = y1 > g.gdim - 1 ? g.gdim - 1 : y1;
    return o;
}

TN_DEV inline bool whole_grid(const Grid& g, Box b) {
    return b.x0 <= 0 && b.y0 <= 0 && b.x1 >= g.gdim - 1 && b.y1 >= g.gdim - 1;
}

// f(p) for every sorted position p in the cells of b that are not in ex.  A row of b is one or two runs of cells
// (left and right of ex) and so one or two ranges of positions; the lanes stride through each range in turn.
template <typename F>
TN_DEV inline void scan_cells(const Grid& g, Box b, Box ex, int lane, F f) {
    for (int cy = b.y0; cy <= b.y1; ++cy) {
        const bool cut = ex.x0 <= ex.x1 && cy >= ex.y0 && cy <= ex.y1;
        for (int part = 0; part < (cut ? 2 : 1); ++part) {
            int lo = b.x0, hi = b.x1;
            if (cut && part == 0) hi = hi < ex.x0 - 1 ? hi : ex.x0 - 1;
            if (cut && part == 1) lo = lo > ex.x1 + 1 ? lo : ex.x1 + 1;
            if (lo > hi) continue;
            const unsigned row = (unsigned)cy * (unsigned)g.gdim;
            const unsigned p1 = g.cell_start[row + hi + 1];
            for (unsigned p = g.cell_start[row + lo] + lane; p < p1; p += TN_WAVE) f(p);
        }
    }
}

struct Cand { int x, y; unsigned p; int ok; };

TN_DEV inline Cand shfl_cand(Cand c, int o) {
    Cand r;
    r.x = TN_SHFL_XOR(c.x, o);
    r.y = TN_SHFL_XOR(c.y, o);
    r.p = TN_SHFL_XOR(c.p, o);
    r.ok = TN_SHFL_XOR(c.ok, o);
    return r;
}

// "m beats k" as the apex of the edge a -> b (both strictly left of it): m lies inside the circle (a, b, k), or on it
// and before k in the walk's sense of rotation about pi.  A strict total order on distinct tracers: it orders the
// circle centres along the bisector of a b, and two cocircular tracers cannot also be collinear with pi.
TN_DEV inline bool beats(Pt a, Pt b, Pt pi, bool ccw, Cand k, Cand m) {
    if (!m.ok) return false;
    if (!k.ok) return true;
    const Pt pk = {k.x, k.y}, pm = {m.x, m.y};
    const i64 v = incircle(a, b, pk, pm);
    if (v != 0) return v > 0;
    return (ccw ? orient(pi, pm, pk) : orient(pi, pk, pm)) > 0;
}

TN_DEV inline Cand wave_best(Pt a, Pt b, Pt pi, bool ccw, Cand best) {
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
        const Cand other = shfl_cand(best, o);
        if (beats(a, b, pi, ccw, best, other)) best = other;
    }
    return best;
}

// The nearest neighbour of the tracer at sorted position si, by growing boxes of cells round its own cell.  After
// the box of radius r cells every tracer not yet seen differs by at least r * cs + 1 pixels on one axis.
TN_DEV inline Cand nearest(const Grid& g, unsigned si, int lane) {
    const Obj oi = g.pts[si];
    const int cx = oi.x / g.cs, cy = oi.y / g.cs;
    Cand best = {0, 0, 0u, 0};
    i64 bd = 0;
    Box seen = {0, 0, -1, -1};
    for (int r = 1;; r *= 2) {
        const Box b = clip_box(g, cx - r, cy - r, cx + r, cy + r);
        scan_cells(g, b, seen, lane, [&](unsigned p) {
            if (p == si) return;
            const Obj o = g.pts[p];
            const i64 dx = o.x - oi.x, dy = o.y - oi.y, d = dx * dx + dy * dy;
            if (!best.ok || d < bd || (d == bd && p < best.p)) { best = Cand{o.x, o.y, p, 1}; bd = d; }
        });
        seen = b;
        for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
            const Cand other = shfl_cand(best, o);
            const i64 od = TN_SHFL_XOR(bd, o);
            if (other.ok && (!best.ok || od < bd || (od == bd && other.p < best.p))) { best = other; bd = od; }
        }
        const i64 reach = (i64)r * g.cs + 1;
        if ((best.ok && bd <= reach * reach) || whole_grid(g, b)) return best;
    }
}

// The apex of the edge pi -> pj: the tracer strictly left of a -> b ((a, b) = (pi, pj) counter-clockwise, (pj, pi)
// clockwise) that beats every other one.  Boxes of cells round the edge grow until one holds a candidate; whatever
// beats that candidate lies in its circle, so the cells under that circle's box complete the search.  ok == 0: no
// tracer is left of the edge (it is on the hull).
TN_DEV inline Cand apex(const Grid& g, Pt pi, Pt pj, bool ccw, int lane) {
    const Pt a = ccw ? pi : pj, b = ccw ? pj : pi;
    const int cxi = pi.x / g.cs, cyi = pi.y / g.cs, cxj = pj.x / g.cs, cyj = pj.y / g.cs;
    Box box = clip_box(g, (cxi < cxj ? cxi : cxj) - 1, (cyi < cyj ? cyi : cyj) - 1, (cxi > cxj ? cxi : cxj) + 1,
                       (cyi > cyj ? cyi : cyj) + 1);
    Box seen = {0, 0, -1, -1};
    Cand best = {0, 0, 0u, 0};
    auto consider = [&](unsigned p) {
        const Obj o = g.pts[p];
        const Pt pm = {o.x, o.y};
        if (orient(a, b, pm) <= 0) return;
        const Cand m = {o.x, o.y, p, 1};
        if (beats(a, b, pi, ccw, best, m)) best = m;
    };
    for (;;) {
        scan_cells(g, box, seen, lane, consider);
        seen = box;
        best = wave_best(a, b, pi, ccw, best);
        if (best.ok || whole_grid(g, box)) break;
        const int w = box.x1 - box.x0 + 1, h = box.y1 - box.y0 + 1, d = w > h ? w : h;
        box = clip_box(g, box.x0 - d, box.y0 - d, box.x1 + d, box.y1 + d);
    }
    if (!best.ok) return best;
    const Pt pk = {best.x, best.y};
    scan_cells(g, circle_box(g, a, b, pk), seen, lane, consider);
    return wave_best(a, b, pi, ccw, best);
}

TN_DEV inline i64 wave_sum(i64 v) {
    for (int o = TN_WAVE / 2; o > 0; o >>= 1) v += TN_SHFL_XOR(v, o);
    return v;
}

// The star of the tracer at sorted position si: counter-clockwise from its nearest neighbour j0 until the star closes
// or the hull is met, then clockwise from j0 to the hull.  Each step finds the apex k of the edge (i, j), then scans
// the cells under the circle (i, j, k) for the tracers on it and inside it, and appends the circle's record when i is
// the smallest index on it and (i, e) is the first edge of i's fan over it.  Lane 0 appends.
TN_DEV inline void walk_star(const Grid& g, unsigned si, int lane, const Out& out) {
    const Obj oi = g.pts[si];
    const Pt pi = {oi.x, oi.y};
    const Cand j0 = nearest(g, si, lane);
    if (!j0.ok) return;
    u64 steps = 0;
    for (int dir = 0; dir < 2; ++dir) {
        const bool ccw = dir == 0;
        Cand j = j0;
        for (;;) {
            if (++steps > 2 * (u64)g.n + 4) {               // a star has fewer edges than there are tracers
                if (lane == 0) TN_ATOMIC_ADD(&out.count[1], 1ull);
                return;
            }
            const Pt pj = {j.x, j.y};
            const Cand k = apex(g, pi, pj, ccw, lane);
            if (!k.ok) break;                               // hull: walk the other way from j0
            const Pt pk = {k.x, k.y};
            const Pt a = ccw ? pi : pj, b = ccw ? pj : pi;  // (a, b, pk) is counter-clockwise
            const Cand e = ccw ? j : k, nxt = ccw ? k : j;
            const Pt pe = {e.x, e.y};
            i64 n_on = 0, n_in = 0, bad = 0;
            unsigned min_id = oi.id;
            scan_cells(g, circle_box(g, a, b, pk), Box{0, 0, -1, -1}, lane, [&](unsigned p) {
                const Obj o = g.pts[p];
                const Pt pm = {o.x, o.y};
                const i64 v = incircle(a, b, pk, pm);
                if (v > 0) ++n_in;
                if (v != 0) return;
                ++n_on;
                min_id = o.id < min_id ? o.id : min_id;
                if (p != si && p != e.p && orient(pi, pe, pm) <= 0) ++bad;
            });
            n_on = wave_sum(n_on);
            n_in = wave_sum(n_in);
            bad = wave_sum(bad);
            for (int o = TN_WAVE / 2; o > 0; o >>= 1) {
                const unsigned other = TN_SHFL_XOR(min_id, o);
                min_id = other < min_id ? other : min_id;
            }
            if (lane == 0) {
                if (n_in != 0) TN_ATOMIC_ADD(&out.count[1], 1ull);
                if (min_id == oi.id && bad == 0) {
                    const Pt pn = {nxt.x, nxt.y};
                    i64 X, Y, W, Ux, Uy;
                    circle(pi, pe, pn, X, Y, W, Ux, Uy);
                    const i64 top = W * (g.npix - 1);
                    if (X >= 0 && X <= top && Y >= 0 && Y <= top) {
                        const u64 slot = TN_ATOMIC_ADD(&out.count[0], 1ull);
                        if (slot < out.cap) {
                            i64* r = out.records + 7 * slot;
                            r[0] = oi.id; r[1] = g.pts[e.p].id; r[2] = g.pts[nxt.p].id; r[3] = n_on;
                            r[4] = X; r[5] = Y; r[6] = W;
                        }
                    }
                }
            }
            j = k;
            if (j.p == j0.p) return;                        // closed star
        }
    }
}

}  // namespace tn
