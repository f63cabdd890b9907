// Reduced-density-matrix pass planner: which kernel, over which kept bits, and
// which list of launches QEngineHIP<R>::GetReducedDensityMatrix takes. Pure
// host code, no HIP includes, so the bindings expose it without a GPU. The
// engine walks exactly the list this returns.
//
// The kernels work on the kept qubits in ascending physical order; the engine
// permutes the result into the caller's order on the host.
//  - Register (k <= QA_RDM_REG_MAX): one pass, every thread keeps the unique
//    entries of rho in double registers.
//  - Tile (k <= QA_RDM_TILE_MAX): one pass, a block stages 2^T amplitudes in
//    LDS, whose address bits are the kept bits plus the lowest environment
//    bits, and every thread owns a 4x4 patch of rho's upper triangle.
//  - Wide: the QA_RDM_TILE_MAX physically lowest kept bits stay in the tile,
//    the others are enumerated as blocks: launch (A, B), A <= B, fixes them to
//    A on the row side and to B on the column side and yields the cross block
//    sum_e psi[e,A,a] conj(psi[e,B,b]). Blocks with A > B are the conjugate
//    transposes. An off-diagonal launch stages two tiles of half the size.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace qrack_amd {

constexpr int QA_RDM_REG_MAX = 3;  // kept qubits of the register kernel
constexpr int QA_RDM_TILE_MAX = 6; // kept qubits inside one tile (KT)
// longest run of rows a tile-kernel thread sums in the engine's real type
// before the run goes into its double accumulators
constexpr int QA_RDM_RUN = 32;
// grid caps: a block leaves one set of double partials, so these bound the
// partials buffer (register: 2048 x 64 doubles = 1 MB at k = 3; tile:
// 1024 x 8192 doubles = 64 MB at k = 6)
constexpr int QA_RDM_REG_GRID = 2048;
constexpr int QA_RDM_TILE_GRID = 1024;

// 4x4 patches of a 2^kt x 2^kt block that a tile launch computes: all of
// them, or the upper triangle when row and column side are the same slice
constexpr int rdmTilePatches(int kt, bool diag)
{
    const int np = (1 << kt) / 4;
    return diag ? np * (np + 1) / 2 : np * np;
}

enum class RdmRegime { Register, Tile, Wide };

struct RdmLaunch {
    uint32_t a; // value of the block bits on the row side
    uint32_t b; // ... on the column side, a <= b
};

struct RdmPlan {
    RdmRegime regime;
    std::vector<int> tileBits;  // kept qubits a launch resolves itself, ascending
    std::vector<int> blockBits; // kept qubits enumerated by the launch list, ascending
    int tileAddrBits;           // T of a launch with a == b (0 in the register regime)
    int crossAddrBits;          // T of each of the two tiles of a launch with a < b
    std::vector<RdmLaunch> launches;
};

inline const char* rdmRegimeName(RdmRegime r)
{
    return r == RdmRegime::Register ? "register" : r == RdmRegime::Tile ? "tile" : "wide";
}

// `qubits` must be distinct and below `width` (validateRdmQubits)
inline RdmPlan rdmPassPlan(int width, const std::vector<int>& qubits, int realBytes)
{
    RdmPlan p;
    std::vector<int> sorted(qubits);
    std::sort(sorted.begin(), sorted.end());
    const int k = (int)sorted.size();
    p.tileAddrBits = 0;
    p.crossAddrBits = 0;
    if (k <= QA_RDM_REG_MAX) {
        p.regime = RdmRegime::Register;
        p.tileBits = sorted;
        p.launches.push_back({ 0u, 0u });
        return p;
    }
    const int kt = std::min(k, QA_RDM_TILE_MAX);
    p.regime = k <= QA_RDM_TILE_MAX ? RdmRegime::Tile : RdmRegime::Wide;
    p.tileBits.assign(sorted.begin(), sorted.begin() + kt);
    p.blockBits.assign(sorted.begin() + kt, sorted.end());
    const int tb = realBytes == 4 ? 12 : 11; // 32 KB of amplitudes
    const int nEnv = width - k;
    p.tileAddrBits = std::min(tb, kt + nEnv);
    p.crossAddrBits = std::min(tb - 1, kt + nEnv);
    const uint32_t nBlocks = 1u << (k - kt);
    for (uint32_t a = 0; a < nBlocks; ++a) {
        for (uint32_t b = a; b < nBlocks; ++b) p.launches.push_back({ a, b });
    }
    return p;
}

} // namespace qrack_amd
