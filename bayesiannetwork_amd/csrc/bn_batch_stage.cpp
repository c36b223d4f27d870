// bn_batch_stage.cpp -- layout and filling of a batch's evidence staging block (bn_batch_stage.hpp).  Host arithmetic only.
#include "bn_batch_stage.hpp"

#include <algorithm>
#include <cstring>

namespace bn_stage {

BatchLayout layout_of(int32_t n_sets, const int32_t* ne, const int32_t* ev_off) {
    BatchLayout l;
    l.n_sets = n_sets;
    l.node_at.assign(size_t(n_sets) + 1, 0);
    l.off_at.assign(size_t(n_sets) + 1, 0);
    l.val_at.assign(size_t(n_sets) + 1, 0);
    for (int32_t q = 0; q < n_sets; ++q) {
        const int64_t cnt = std::max(ne[q], 0);
        l.node_at[q + 1] = l.node_at[q] + cnt;
        l.off_at[q + 1] = l.off_at[q] + cnt + 1;
        l.val_at[q + 1] = l.val_at[q] + (cnt > 0 && ev_off ? ev_off[l.off_at[q] + cnt] : 0);
    }
    l.b_node = 0;
    l.b_off = size_t(l.node_at[n_sets]) * 4;
    l.b_val = (l.b_off + size_t(l.off_at[n_sets]) * 4 + 7) & ~size_t(7);
    l.b_meta = l.b_val + size_t(l.val_at[n_sets]) * 8;
    l.bytes = l.b_meta + size_t(n_sets) * kMetaWords * 4;
    return l;
}

void BatchLayout::fill(char* dst, const int32_t* ev_node, const int32_t* ev_off, const double* ev_val) const {
    if (node_at[n_sets] > 0) {
        std::memcpy(dst + b_node, ev_node, size_t(node_at[n_sets]) * 4);
        std::memcpy(dst + b_val, ev_val, size_t(val_at[n_sets]) * 8);
    }
    if (ev_off) std::memcpy(dst + b_off, ev_off, size_t(off_at[n_sets]) * 4);
    int32_t* m = meta(dst);
    for (int32_t q = 0; q < n_sets; ++q, m += kMetaWords) {
        m[0] = int32_t(node_at[q + 1] - node_at[q]); m[1] = int32_t(node_at[q]); m[2] = int32_t(off_at[q]); m[3] = int32_t(val_at[q]);
        m[4] = int32_t(val_at[q + 1] - val_at[q]); m[5] = m[6] = m[7] = 0;
    }
}

}  // namespace bn_stage
