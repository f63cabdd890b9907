// Dense k-qubit gate (MtrxN) planner: the route, the tile a workgroup stages,
// how tiles are enumerated under controls, and the index maps the kernel
// k_mtrx_n uses. Pure host code apart from the QA_HD index maps, no HIP
// includes, so the bindings expose it without a GPU. The engine launches
// exactly the geometry this returns.
//
// Tile bit set S: the targets plus the lowest other bits, until
// |S| = min(n, tile bits). The low contiguous bits of S form the run, so a
// workgroup's global loads and stores are runs of 2^run amplitudes wherever
// the targets sit; with all targets low S is the contiguous tile of the other
// LDS kernels. A control outside S fixes a bit of the tile base, so only
// 2^(n - |S| - cHigh) tiles are visited; a control inside S is a predicate on
// the orbit index.
//
// LDS layout: local index l (bit b of l is the value of the b-th lowest bit of
// S) splits into the target bits j (k bits) and the orbit bits o (|S| - k
// bits). The amplitude sits at (j << oBits) | (o ^ swz(j)): for a fixed matrix
// column consecutive orbits are consecutive slots, whatever the targets, so
// the mat-vec phase reads and writes without bank conflicts and needs no
// per-column bit deposit. The XOR with swz(j) spreads the staging phase, where
// consecutive lanes walk j when the targets are low. Every map here is linear
// over XOR, so a thread forms an address as map(thread part) ^ map(trip part).
#pragma once

#include "../common/types.hpp"

#include <algorithm>
#include <vector>

namespace qrack_amd {

constexpr int QA_MTRXN_TILE_MAX = 12; // most bits of S (fp32; fp64 has 11)
constexpr int QA_MTRXN_MAX_INS = 32;  // S bits above the run + controls outside S
constexpr int QA_MTRXN_BLOCK = 256;   // threads of a workgroup

enum class MtrxNRoute { Apply2x2, Mtrx2q, MtrxN };

inline const char* mtrxnRouteName(MtrxNRoute r)
{
    return r == MtrxNRoute::Apply2x2 ? "apply2x2" : r == MtrxNRoute::Mtrx2q ? "mtrx_2q" : "mtrx_n";
}

// what the kernel needs to know about one call; passed by value
struct MtrxNGeom {
    bitCapInt nTiles;
    bitCapInt baseFixed;                // controls outside S that must be set
    bitCapInt insPow[QA_MTRXN_MAX_INS]; // ascending, all >= 2^run: zero bits of a tile base
    int nIns;
    int m;                         // |S|
    int run;                       // low contiguous bits of S
    int k;                         // targets
    int sHigh[QA_MTRXN_TILE_MAX];  // global bit of local bit run + g
    int lt[QA_MTRXN_MAX];          // local bit of target g, ascending
    unsigned cMaskO;               // in-tile controls, as bits of the orbit index
    unsigned cValO;                // value they must have
};

// swizzle of the orbit field by the target field: K <= 5 puts j above the
// orbit bits that 32 consecutive lanes of the staging loop already walk
QA_HD inline unsigned mtrxnSwz(int k, unsigned j)
{
    return k <= 5 ? (j << (5 - k)) : ((j ^ (j >> 5)) & 31u);
}

// global index of tile t's first amplitude
QA_HD inline bitCapInt mtrxnTileBase(const MtrxNGeom& g, bitCapInt t)
{
    bitCapInt b = t << g.run;
    for (int i = 0; i < g.nIns; ++i) {
        const bitCapInt p = g.insPow[i];
        b = ((b & ~(p - 1u)) << 1u) | (b & (p - 1u));
    }
    return b | g.baseFixed;
}

// offset of local index l from the tile base
QA_HD inline bitCapInt mtrxnGlobalOff(const MtrxNGeom& g, unsigned l)
{
    bitCapInt off = l & ((1u << g.run) - 1u);
    for (int i = 0; i < g.m - g.run; ++i) {
        off |= (bitCapInt)((l >> (g.run + i)) & 1u) << g.sHigh[i];
    }
    return off;
}

// LDS slot of (column or row j, orbit o)
QA_HD inline unsigned mtrxnSlot(int k, int oBits, unsigned j, unsigned o)
{
    return (j << oBits) | (o ^ (mtrxnSwz(k, j) & ((1u << oBits) - 1u)));
}

// LDS slot of local index l
QA_HD inline unsigned mtrxnLdsAddr(const MtrxNGeom& g, unsigned l)
{
    unsigned j = 0, o = l;
    for (int t = g.k - 1; t >= 0; --t) {
        const int b = g.lt[t];
        j |= ((l >> b) & 1u) << t;
        o = ((o >> (b + 1)) << b) | (o & ((1u << b) - 1u));
    }
    return mtrxnSlot(g.k, g.m - g.k, j, o);
}

struct MtrxNPlan {
    MtrxNRoute route;
    MtrxNGeom geom;
    std::vector<int> targets;  // ascending
    std::vector<int> order;    // targets[g] == qubits[order[g]]
    std::vector<int> tileBits; // S, ascending
    int cHigh;                 // controls outside S
    bitCapInt orbitsPerTile;
    int rowsPerThread;
    bool matrixInKernarg;
};

// output rows one thread accumulates: a whole orbit, or the share that keeps
// 256 threads busy on a full tile
constexpr int mtrxnRowsPerThread(int k, int tileBitsMax)
{
    return (1 << k) < (1 << (tileBitsMax - 8)) ? (1 << k) : (1 << (tileBitsMax - 8));
}

// `qubits` and `controls` must have passed validateMtrxN for width n
inline MtrxNPlan mtrxnPlan(int n, const std::vector<int>& qubits, const std::vector<int>& controls,
    bool anti, int realBytes)
{
    MtrxNPlan p;
    const int k = (int)qubits.size();
    p.order.resize(k);
    for (int g = 0; g < k; ++g) p.order[g] = g;
    std::sort(p.order.begin(), p.order.end(), [&](int a, int b) { return qubits[a] < qubits[b]; });
    for (int g = 0; g < k; ++g) p.targets.push_back(qubits[p.order[g]]);
    p.route = k == 1 ? MtrxNRoute::Apply2x2
        : (k == 2 && controls.empty()) ? MtrxNRoute::Mtrx2q
                                       : MtrxNRoute::MtrxN;

    const int tb = realBytes == 4 ? 12 : 11; // 32 KB of amplitudes
    const int m = std::min(n, tb);
    std::vector<bool> inS(n, false);
    for (int t : p.targets) inS[t] = true;
    int have = k;
    for (int b = 0; b < n && have < m; ++b) {
        if (!inS[b]) {
            inS[b] = true;
            ++have;
        }
    }
    for (int b = 0; b < n; ++b) {
        if (inS[b]) p.tileBits.push_back(b);
    }

    MtrxNGeom& g = p.geom;
    g = MtrxNGeom{};
    g.m = m;
    g.k = k;
    g.run = 0;
    while (g.run < m && p.tileBits[g.run] == g.run) ++g.run;
    std::vector<bitCapInt> ins;
    for (int i = g.run; i < m; ++i) {
        g.sHigh[i - g.run] = p.tileBits[i];
        ins.push_back(pow2((bitLenInt)p.tileBits[i]));
    }
    for (int t = 0; t < k; ++t) {
        g.lt[t] = (int)(std::find(p.tileBits.begin(), p.tileBits.end(), p.targets[t]) - p.tileBits.begin());
    }
    p.cHigh = 0;
    for (int c : controls) {
        if (inS[c]) {
            const int lp = (int)(std::find(p.tileBits.begin(), p.tileBits.end(), c) - p.tileBits.begin());
            int below = 0;
            for (int t = 0; t < k; ++t) below += g.lt[t] < lp ? 1 : 0;
            g.cMaskO |= 1u << (lp - below);
        } else {
            ins.push_back(pow2((bitLenInt)c));
            if (!anti) g.baseFixed |= pow2((bitLenInt)c);
            ++p.cHigh;
        }
    }
    g.cValO = anti ? 0u : g.cMaskO;
    if (ins.size() > (size_t)QA_MTRXN_MAX_INS) throw QrackError("MtrxN: too many control qubits");
    std::sort(ins.begin(), ins.end());
    g.nIns = (int)ins.size();
    for (int i = 0; i < g.nIns; ++i) g.insPow[i] = ins[i];
    g.nTiles = pow2((bitLenInt)(n - m - p.cHigh));

    p.orbitsPerTile = pow2((bitLenInt)(m - k));
    p.rowsPerThread = mtrxnRowsPerThread(k, tb);
    p.matrixInKernarg = k <= 3;
    return p;
}

// the matrix in the kernel's basis (targets ascending): a pure permutation of
// rows and columns, no arithmetic
template <typename T>
inline void mtrxnPermuteMatrix(const MtrxNPlan& p, const T* in, T* out)
{
    const int k = (int)p.targets.size();
    const int D = 1 << k;
    std::vector<int> src(D, 0);
    for (int s = 0; s < D; ++s) {
        for (int g = 0; g < k; ++g) {
            if ((s >> g) & 1) src[s] |= 1 << p.order[g];
        }
    }
    for (int r = 0; r < D; ++r) {
        for (int c = 0; c < D; ++c) out[r * D + c] = in[src[r] * D + src[c]];
    }
}

// Walks every (tile, local index) the kernel touches, with the kernel's own
// index maps: true when the global indices are exactly the amplitudes the
// out-of-tile controls admit, each once and in range, with the target bits
// where the LDS layout says, and the LDS slots of a tile are a permutation.
// For tests; the cost is 2^n.
inline bool mtrxnPlanCovers(const MtrxNPlan& p, int n, const std::vector<int>& controls, bool anti)
{
    const MtrxNGeom& g = p.geom;
    const bitCapInt N = pow2((bitLenInt)n);
    const unsigned tileLen = 1u << g.m;
    const int oBits = g.m - g.k;
    bitCapInt highMask = 0;
    for (int c : controls) {
        if (std::find(p.tileBits.begin(), p.tileBits.end(), c) == p.tileBits.end()) {
            highMask |= pow2((bitLenInt)c);
        }
    }
    const bitCapInt highVal = anti ? 0 : highMask;
    std::vector<unsigned char> seen(N, 0);
    bitCapInt count = 0;
    for (bitCapInt t = 0; t < g.nTiles; ++t) {
        const bitCapInt base = mtrxnTileBase(g, t);
        std::vector<unsigned char> slot(tileLen, 0);
        for (unsigned l = 0; l < tileLen; ++l) {
            const bitCapInt i = base + mtrxnGlobalOff(g, l);
            if (i >= N || seen[i] || (i & highMask) != highVal) return false;
            seen[i] = 1;
            ++count;
            const unsigned a = mtrxnLdsAddr(g, l);
            if (a >= tileLen || slot[a]) return false;
            slot[a] = 1;
            // the slot's row field is the targets' value, its orbit field
            // carries the in-tile controls
            const unsigned j = a >> oBits;
            const unsigned o = (a & ((1u << oBits) - 1u)) ^ (mtrxnSwz(g.k, j) & ((1u << oBits) - 1u));
            if (mtrxnSlot(g.k, oBits, j, o) != a) return false;
            for (int q = 0; q < g.k; ++q) {
                if (((i >> p.targets[q]) & 1u) != ((j >> q) & 1u)) return false;
            }
            bool inCtl = true;
            for (int c : controls) {
                if (((i >> c) & 1u) != (anti ? 0u : 1u)) inCtl = false;
            }
            if (inCtl != ((o & g.cMaskO) == g.cValO)) return false;
        }
    }
    return count == (N >> p.cHigh);
}

} // namespace qrack_amd
