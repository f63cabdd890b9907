// QFT pass planner: which kernels, over which columns, a start-0 QFT of
// `length` qubits takes on the HIP engine. Pure host code, no HIP includes,
// so the bindings expose it without a GPU. QEngineHIP<R>::QFT walks the
// list top-down; IQFT walks it backwards with every pass adjointed, so the
// inverse is always the exact mirror of the forward schedule.
#pragma once

#include <algorithm>
#include <array>
#include <climits>
#include <vector>

namespace qrack_amd {

enum class QftPassKind {
    Low, // low ladder: columns nCols-1..0 inside contiguous LDS tiles
    Mid, // 2D LDS tile pass; nCols <= 6 on the 64-wide kernel, 8/9 on the wide one
    Col  // nCols (1..5) fused register columns, one state pass; column 0 alone is an H
};

struct QftPass {
    QftPassKind kind;
    int colLo; // lowest column of the pass
    int nCols; // columns colLo .. colLo+nCols-1
};

// mid-pass widths: on the 64-amplitude-run kernel, and on the wide-tile one
constexpr int QA_QFT_MID_LOWBITS = 6;
constexpr int QA_QFT_WIDE_MIN_COLS = 8;
constexpr int QA_QFT_WIDE_MAX_COLS = 9;

struct QftPlanOpts {
    bool ldsLow = true;   // QRACK_GPU_QFT_LDS
    bool ldsMid = true;   // QRACK_GPU_QFT_MIDLDS (fp32 only, whatever is asked)
    int fuseMax = 4;      // QRACK_GPU_QFT_FUSE
    int midMax = 9;       // QRACK_GPU_QFT_MIDMAX; <= 7 leaves only the 64-wide kernel
    int wideLowBits = 4;  // contiguous-run bits of the wide kernel (colLo bound)
};

namespace qftplan {

// register-column pass the fused kernels take with `i` columns left
inline int fusedCols(int i, int width, int fuseMax)
{
    const int col = i - 1;
    if (fuseMax >= 5 && col >= 4 && width >= 6) return 5;
    if (fuseMax >= 4 && col >= 3 && width >= 5) return 4;
    if (fuseMax >= 3 && col >= 2 && width >= 4) return 3;
    if (fuseMax >= 2 && col >= 1 && width >= 3) return 2;
    return 1;
}

// The six-columns-at-a-time schedule: mid passes of 6 (a trailing 5 takes
// a full 6 dipping one column below the tile boundary), a trailing 4/3/2 as
// one uniform group, then the K-aligned low ladder under peeled columns.
inline std::vector<QftPass> greedy(int length, bool lds, bool mid, int tb, int AK, int width,
    int fuseMax)
{
    std::vector<QftPass> plan;
    int i = length;
    while (i > 0) {
        if (lds && i <= tb) {
            const int r = i % AK;
            if (!r) {
                plan.push_back({ QftPassKind::Low, 0, i });
                break;
            }
            if (i != r) {
                plan.push_back({ QftPassKind::Col, i - r, r });
                i -= r;
                continue;
            }
        }
        if (lds && mid && i > tb) {
            const int rem = i - tb;
            const int nc = rem >= 5 ? 6 : rem;
            if (nc >= 2 && i - nc >= QA_QFT_MID_LOWBITS) {
                plan.push_back({ QftPassKind::Mid, i - nc, nc });
                i -= nc;
                continue;
            }
        }
        const int k = fusedCols(i, width, fuseMax);
        plan.push_back({ QftPassKind::Col, i - k, k });
        i -= k;
    }
    return plan;
}

} // namespace qftplan

// Pass list, top column first, for a QFT over bits start..start+length-1 of a
// `width`-qubit engine whose real type has `realBytes` bytes.
//
// With no wide width allowed (midMax < 8) this is the six-at-a-time
// schedule above. Otherwise a search over
//   - a low ladder of i columns (i <= tile bits, i a multiple of the ladder K),
//   - a mid pass of 2/3/4/6 columns (colLo >= 6) or 8/9 columns (colLo >=
//     wideLowBits) whose top column is above the low tile,
//   - 1..fuseMax fused register columns
// takes the fewest state passes; among equals the fewest wide passes, then
// the fewest 8-column (K=4) ones. The six-at-a-time schedule is kept unless
// the search is strictly better under that order.
inline std::vector<QftPass> qftPassPlan(
    int length, int start, int width, int realBytes, const QftPlanOpts& o = QftPlanOpts())
{
    const int tb = realBytes == 4 ? 12 : 11;
    const int AK = realBytes == 4 ? 4 : 3;
    const bool lds = o.ldsLow && start == 0 && width >= tb;
    const bool mid = o.ldsMid && realBytes == 4;
    std::vector<QftPass> base = qftplan::greedy(length, lds, mid, tb, AK, width, o.fuseMax);
    const int wideMax = std::min(o.midMax, QA_QFT_WIDE_MAX_COLS);
    if (!lds || !mid || wideMax < QA_QFT_WIDE_MIN_COLS || length <= tb) return base;

    using Cost = std::array<int, 3>; // passes, wide passes, 8-column wide passes
    const Cost inf{ INT_MAX, INT_MAX, INT_MAX };
    std::vector<Cost> best(length + 1, inf);
    std::vector<QftPass> step(length + 1, QftPass{ QftPassKind::Col, 0, 0 });
    best[0] = Cost{ 0, 0, 0 };
    auto consider = [&](int i, QftPass p, int rest, Cost add) {
        if (best[rest] == inf) return;
        const Cost c{ best[rest][0] + add[0], best[rest][1] + add[1], best[rest][2] + add[2] };
        if (c < best[i]) {
            best[i] = c;
            step[i] = p;
        }
    };
    const int narrow[4] = { 6, 4, 3, 2 };
    for (int i = 1; i <= length; ++i) {
        if (i <= tb && (i % AK) == 0) consider(i, { QftPassKind::Low, 0, i }, 0, { 1, 0, 0 });
        if (i > tb) {
            // among plans of equal cost the first found stays: wide on top
            for (int nc = wideMax; nc >= QA_QFT_WIDE_MIN_COLS; --nc) {
                if (i - nc >= o.wideLowBits) {
                    consider(i, { QftPassKind::Mid, i - nc, nc }, i - nc, { 1, 1, nc == 8 ? 1 : 0 });
                }
            }
            for (int nc : narrow) {
                if (i - nc >= QA_QFT_MID_LOWBITS) {
                    consider(i, { QftPassKind::Mid, i - nc, nc }, i - nc, { 1, 0, 0 });
                }
            }
        }
        const int kMax = std::min({ i, std::max(1, std::min(o.fuseMax, 5)), std::max(1, width - 1) });
        for (int k = kMax; k >= 1; --k) {
            consider(i, { QftPassKind::Col, i - k, k }, i - k, { 1, 0, 0 });
        }
    }
    const Cost baseCost{ (int)base.size(), 0, 0 };
    if (!(best[length] < baseCost)) return base;
    std::vector<QftPass> plan;
    for (int i = length; i > 0; i = step[i].colLo) {
        plan.push_back(step[i]);
        if (step[i].kind == QftPassKind::Low) break;
    }
    return plan;
}

// ---- support-restricted passes of a transform applied to a basis state ------
//
// A QFT column is an H and a phase ladder controlled by lower bits; applied to
// phase·|p> the state stays a product state, so after the columns C of some
// passes an amplitude x can be nonzero only where ((x ^ p) & ~F) == 0, F the
// union of those C ("free" bits). A pass then has to visit only the tiles
// whose tile-index bits outside F equal p's, and to take its first-group input
// from the buffer only inside that support (+0 elsewhere). Every pass but the
// last writes its active tiles whole; the last visits every tile, so the
// buffer is fully defined on return.

struct QftSupportPass {
    QftPass pass;
    int lowBits;             // contiguous-run bits of the pass's tile
    int tileIndexBits;       // width - tile bits
    unsigned long long fixedMask; // ~F on entry: input nonzero only where ((x ^ p) & fixedMask) == 0
    bool fromBuffer;         // F non-empty on entry: in-support input is loaded, not basisPhase
    unsigned long long tileFree;  // tile-index bits the pass iterates over
    unsigned long long tileFixed; // value of the other tile-index bits
    unsigned long long activeTiles; // 2^popcount(tileFree)
};

struct QftSupportPlan {
    bool eligible = false;
    std::vector<QftSupportPass> passes; // in execution order
};

namespace qftplan {

// tile index of amplitude x (or of a mask of x bits) in a pass's tiling
inline unsigned long long tileIndexOf(
    unsigned long long x, const QftPass& p, int lowBits)
{
    if (p.kind == QftPassKind::Low) return x >> lowBits;
    const unsigned long long midMask = (1ull << (p.colLo - lowBits)) - 1ull;
    return ((x >> (p.colLo + p.nCols)) << (p.colLo - lowBits)) | ((x >> lowBits) & midMask);
}

} // namespace qftplan

// Support schedule of `plan` (from qftPassPlan, forward order) run forwards
// or, inverse, backwards on phase·|perm>. Eligible only for a start-0
// full-width transform of at least two passes, all of them Low or Mid.
inline QftSupportPlan qftSupportPlan(const std::vector<QftPass>& plan, int length, int start,
    int width, int realBytes, unsigned long long perm, bool inverse, int wideLowBits = 4)
{
    QftSupportPlan out;
    // (mid passes, and so every multi-pass plan without a Col pass, are fp32-only)
    if (realBytes != 4 || start != 0 || length != width || width >= 63 || plan.size() < 2u) {
        return out;
    }
    for (const QftPass& p : plan) {
        if (p.kind != QftPassKind::Low && p.kind != QftPassKind::Mid) return out;
    }
    const int tb = realBytes == 4 ? 12 : 11;
    const unsigned long long all = (1ull << width) - 1ull;
    unsigned long long freeBits = 0;
    const size_t n = plan.size();
    for (size_t k = 0; k < n; ++k) {
        const QftPass& p = inverse ? plan[n - 1 - k] : plan[k];
        QftSupportPass s;
        s.pass = p;
        s.lowBits = p.kind == QftPassKind::Low ? tb
            : p.nCols >= QA_QFT_WIDE_MIN_COLS  ? wideLowBits
                                               : QA_QFT_MID_LOWBITS;
        const int tileBits = p.kind == QftPassKind::Low ? tb : s.lowBits + p.nCols;
        if (tileBits > width || (p.kind == QftPassKind::Mid && p.colLo < s.lowBits)) {
            return QftSupportPlan();
        }
        s.tileIndexBits = width - tileBits;
        s.fixedMask = all & ~freeBits;
        s.fromBuffer = freeBits != 0;
        const unsigned long long allTiles = (1ull << s.tileIndexBits) - 1ull;
        if (k + 1 == n) {
            s.tileFree = allTiles;
            s.tileFixed = 0;
        } else {
            s.tileFree = qftplan::tileIndexOf(freeBits, p, s.lowBits) & allTiles;
            s.tileFixed = qftplan::tileIndexOf(perm & all, p, s.lowBits) & allTiles & ~s.tileFree;
        }
        s.activeTiles = 1ull << __builtin_popcountll(s.tileFree);
        out.passes.push_back(s);
        freeBits |= ((1ull << p.nCols) - 1ull) << p.colLo;
    }
    out.eligible = true;
    return out;
}

// ---- last low pass of a support plan: the orbits that hold a nonzero --------
//
// Entering the forward last pass (a low ladder of nCols columns, K = 4 column
// groups from gLo = nCols-4 down to 0) a tile is nonzero only where the
// in-tile index agrees with perm in its nCols low bits: one amplitude for 12
// columns, sixteen for 8. A group's 16-point orbit is the set of indices that
// differ only in bits gLo..gLo+3; `below` is its bits under gLo. Group by
// group the nonzeros spread over bits gLo..gLo+3, so in the group at gLo
// exactly the orbits with below == perm's bits under gLo have a nonzero
// input, (tile / 16) >> gLo of them per tile, and it sits in slot
// (perm >> gLo) & 15. Every other orbit transforms sixteen zeros.

struct QftSparseLastGroup {
    int gLo;        // lowest column of the group
    int realOrbits; // orbits per tile with a nonzero input
    int below;      // their `below` value
    int slot;       // slot of the nonzero input inside each of them
};

struct QftSparseLastPlan {
    bool eligible = false;
    std::vector<QftSparseLastGroup> groups; // in execution order, gLo descending
};

inline QftSparseLastPlan qftSparseLastPlan(int nCols, unsigned long long perm)
{
    constexpr int tb = 12; // fp32 tile bits
    constexpr int K = 4;   // fp32 ladder group width
    QftSparseLastPlan out;
    if (nCols != 8 && nCols != 12) return out;
    for (int gLo = nCols - K; gLo >= 0; gLo -= K) {
        QftSparseLastGroup g;
        g.gLo = gLo;
        g.realOrbits = (1 << (tb - K)) >> gLo;
        g.below = (int)(perm & ((1ull << gLo) - 1ull));
        g.slot = (int)((perm >> gLo) & ((1ull << K) - 1ull));
        out.groups.push_back(g);
    }
    out.eligible = true;
    return out;
}

} // namespace qrack_amd
