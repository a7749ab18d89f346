// Argument block shared by the aggregation kernels: the CSR gather kernels (agg.hip) and the matrix-core kernel over
// the bit adjacency (aggm.hip).  One struct, filled by agg_args() below, so either path takes it.
#pragma once
#include "gnm_common.h"
#include <string.h>

struct AggArgs {
    const int32_t* rowptr;     // gather structure arena (forward CSR, or transposed for backward)
    const uint16_t* col;       // graph-local column ids
    const int64_t* b_rp_off;   // [B] offset of graph b's rowptr block
    const int64_t* b_col_off;  // [B] offset of graph b's col block
    const int32_t* deg_rowptr; // forward CSR rowptr arena (degrees for the backward pre-scale)
    const int64_t* b_deg_off;  // [B]
    const int32_t* node_off;   // [B+1] first row of each graph in the batch
    const float* x;
    float* y;
    const float* eps;          // device pointer to eps[layer], or null
    const float* hfwd;         // backward: forward input of the layer (for d eps), or null
    double* deps_partial;      // [B * nslices] or null
    int ldx, ldy, ldh;
    int F;                     // valid feature width
    int nslices;
    int average, self_loop, backward;
    // optional fusion (backward; one 64-wide slice or 32-float slices): y is the gradient arriving at relu(bn(sZ))
    // of the layer below -- add the readout / discriminator terms, apply that ReLU mask, write G and reduce the
    // BatchNorm-backward sums (replaces gnm_bn_relu_bwd_stats for that BatchNorm)
    const float* sZ; const float* s_scale; const float* s_shift; const float* s_mean; const float* s_rstd;
    const float* s_dpool; const float* s_dsc1; const float* s_U; const int32_t* s_inv_perm; const float* s_s2sum;
    double* s_partial;         // [B][2][F]
    int ldsz, ld_dpool, ld_U, s_avg, n_batch;
    // on entry to the launcher: the batch's largest nnz (0 = unknown).  In the kernel: 1 = the graph's column ids are
    // staged in LDS (16-float slices), 2 = the waves have an id scratch in LDS (32-float slices), 0 = neither
    int ids_in_lds;
    int debug;                 // tuning only (GNM_AGG16_DEBUG): 1 no id loads, 2 no epilogue/store, 4 no combine
    unsigned long long* stamps;   // tuning only: per-wave s_memtime stamps, [workgroup][16 waves][64] (gnm_debug_set_stamps)
    // forward prologue (one 64-wide slice or 32-float slices): the input is Z of the previous layer's last Linear; the tile load applies that
    // layer's outer BatchNorm + ReLU, writes the activation h (p_hout) and its graph readout (p_gf) on the way
    const float* p_scale; const float* p_shift;
    float* p_hout; float* p_gf;
    int p_ldh, p_ldgf, p_gf_avg;
    // bit adjacency (aggm.hip only): graph b's [32 W][W] words, W = ceil(n / 32), at adj_bits + b_bits_off[b]
    const uint32_t* adj_bits; const int64_t* b_bits_off;
    int n_graphs, n16_max;     // aggm.hip: B (the grid is padded to whole XCD rounds) and ceil(n_max / 16) * 16
};

// What every aggregation entry fills the same way: the gather structure, the degree CSR (null: the gather's own, as
// for symmetric graphs and the forward), input / output, eps and the d-eps operands, one slice, the mode.  Every other
// field is zero; an entry then sets its own (prologue or epilogue, bit adjacency, slicing).
static inline AggArgs agg_args(const int32_t* rowptr, const uint16_t* col, const int64_t* b_rp_off,
                               const int64_t* b_col_off, const int32_t* deg_rowptr, const int64_t* b_deg_off,
                               const int32_t* node_off, const float* x, int ldx, float* y, int ldy, int F,
                               const float* eps, int average, int self_loop, int backward, const float* hfwd, int ldh,
                               double* deps_partial) {
    AggArgs a;
    memset(&a, 0, sizeof(a));
    a.rowptr = rowptr; a.col = col; a.b_rp_off = b_rp_off; a.b_col_off = b_col_off;
    a.deg_rowptr = deg_rowptr ? deg_rowptr : rowptr;
    a.b_deg_off = b_deg_off ? b_deg_off : b_rp_off;
    a.node_off = node_off; a.x = x; a.y = y; a.eps = eps; a.hfwd = hfwd; a.deps_partial = deps_partial;
    a.ldx = ldx; a.ldy = ldy; a.ldh = ldh; a.F = F; a.nslices = 1;
    a.average = average; a.self_loop = self_loop; a.backward = backward;
    return a;
}
