// bn_info.hpp -- entropy and all-pairs mutual information over a pattern table (reference
// bayesian/evaluation/transinformation.hpp).  Host-side view of the kernels in bn_info_kernels.hip;
// the C ABI (bn_info_* of include/bn_mi355x.h) is in bn_info.cpp.
#pragma once

#include <cstdint>

namespace bnmi {

constexpr int kInfoChunkShift = 12;            // cells are summed in chunks of 4096 consecutive keys
constexpr int kInfoMaxKeyVars = 64;            // a <= 64-bit key has at most 64 columns of arity >= 2
constexpr int kInfoTile = 128;                 // all-pairs workgroup tile (slot columns)
constexpr int kInfoPatternAlign = 64;          // patterns per row of the transposed table, rounded up
constexpr int64_t kInfoSegment = int64_t(1) << 24;  // i32 flush period: 127 * 2^24 < 2^31
constexpr uint64_t kInfoDenseMaxCells = uint64_t(1) << 22;

// the resident table: transposed states [n][Ppad] and the occurrence counts
struct InfoDev {
    int32_t n;
    int64_t P, Ppad;
    int32_t D;                              // 7-bit digit planes of the counts
    const uint8_t* T;                       // [n][Ppad], zero beyond P
    const unsigned long long* w;            // [P]
    const uint8_t* wd;                      // [D][Ppad], digit d of each count, zero beyond P
};

// a canonical set: table columns in increasing order, arity >= 2 (arity-1 columns add no key digit)
struct InfoSet {
    int32_t nv;
    int32_t col[kInfoMaxKeyVars];
    int32_t k[kInfoMaxKeyVars];
};

struct PairArgs {
    const uint8_t* T;
    int64_t Ppad;
    const uint8_t* wd;
    int32_t D;
    int32_t ntile;                          // Kpad / kInfoTile
    const int32_t* colinfo;                 // [Kpad] (table column << 8) | state; padding: state 255 of column 0
    const int32_t* colvar;                  // [Kpad] slot variable owning the column, -1 for padding
    const int32_t* sv_start;                // [slot vars] first slot column
    const int32_t* sv_k;                    // [slot vars] arity
    const int32_t* sv_col;                  // [slot vars] table column
    const int32_t* sv_user;                 // [slot vars] position in the caller's list
    int32_t m;
    double Nd;
    double* hxy;                            // [m][m]
    double* h;                              // [m]
    const int64_t* dump_off;                // [m][m] offset of the block in `dump`, -1: not wanted (null: no dump)
    unsigned long long* dump;
    // the conditional form (null / 0: unconditional): the conditioning column's row of T and its arity; then hxy, h and dump hold
    // H(X, Y, Z), H(X, Z) and the blocks [kz][k_x][k_y]
    const uint8_t* zrow;
    int32_t kz;
};

// each returns a hipError_t value (0: success)
int info_launch_transpose(const uint8_t* raw, int64_t P, int32_t n, int64_t Ppad, const int32_t* k, uint8_t* T,
                          unsigned* bad, void* stream);
int info_launch_digits(const unsigned long long* w, int64_t P, int64_t Ppad, int32_t D, uint8_t* wd, void* stream);
// H of one canonical set.  route 1: dense cells [ncells]; route 2: sort on the packed key (key_bits wide).
// cells_out (host, route 1 only, may be null): the cell counts in key order.
int info_entropy_run(const InfoDev& t, const InfoSet& s, int route, uint64_t ncells, int key_bits, double Nd,
                     double* h_out, unsigned long long* cells_out, void* stream);
int info_launch_pairs(const PairArgs& a, bool flush, void* stream);
// mi[x][y] = h[x] + h[y] - hxy[x][y] over [m][m] on the device (transinformation.hpp:60): the arithmetic bn_info_pair_entropies
// does on the host, so the same bits
int info_launch_mi(const double* h, const double* hxy, int32_t m, double* mi, void* stream);
// cmi[x][y] = hxz[x] + hxz[y] - hxyz[x][y] - hz over [m][m] on the device, left to right
int info_launch_cmi(const double* hxz, const double* hxyz, int32_t m, double hz, double* cmi, void* stream);

}  // namespace bnmi
