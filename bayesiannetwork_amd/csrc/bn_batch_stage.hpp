// bn_batch_stage.hpp -- the staging block of a batch's evidence (bn_bp_set_evidence_batch): [nodes | offs | vals | per-set meta], as the
// kernels read it (bn_small.hip, bn_mid.hip: the whole arrays + the meta words; the evidence kernels: one set's slices).  Where each
// array and each set's entries start, filling the block and the pointers of one set are pure host functions: no HIP, no engine --
// tests/cpp/test_batch_plan.cpp compiles this with bn_batch_stage.cpp alone.
#ifndef BN_BATCH_STAGE_HPP
#define BN_BATCH_STAGE_HPP
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bn_stage __attribute__((visibility("hidden"))) {

constexpr int kMetaWords = 8;   // per set {count, first node entry, first offset entry, first value, values, 0, 0, 0}

// evidence set q inside a block at some base address (host or device: the block is copied whole)
struct SetView {
    int32_t ne = 0;
    int32_t* node = nullptr;
    int32_t* off = nullptr;
    double* val = nullptr;
};

struct BatchLayout {
    int32_t n_sets = 0;
    std::vector<int64_t> node_at, off_at, val_at;        // [n_sets + 1]: set q's first entry in the concatenated arrays; [n_sets] = the totals
    size_t b_node = 0, b_off = 0, b_val = 0, b_meta = 0; // byte offsets of the four parts (b_val: 8-byte aligned)
    size_t bytes = 0;

    // the caller's concatenated arrays -> the block at dst (ev_off may be null when no set has a finding; then the offsets stay unwritten)
    void fill(char* dst, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val) const;
    SetView set_view(char* base, int32_t q) const {
        return {int32_t(node_at[q + 1] - node_at[q]), reinterpret_cast<int32_t*>(base + b_node) + node_at[q],
                reinterpret_cast<int32_t*>(base + b_off) + off_at[q], reinterpret_cast<double*>(base + b_val) + val_at[q]};
    }
    int32_t* meta(char* base) const { return reinterpret_cast<int32_t*>(base + b_meta); }
};

// ne[q] findings per set, ne[q] + 1 offsets per set (ev_off, concatenated; the last one of a set = its number of values).  Meant for
// validated input; so that a caller may validate set by set with the offsets in hand, a negative count reads as 0 and a null ev_off
// as "no values": everything in front of the first such set is as for valid input.
BatchLayout layout_of(int32_t n_sets, const int32_t* ne, const int32_t* ev_off);

}  // namespace bn_stage

#endif  // BN_BATCH_STAGE_HPP
