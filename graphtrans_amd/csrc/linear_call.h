// linear_call.h — the call records of the Linear GEMM dispatchers (linear.hip).  One record carries everything one GEMM call was asked
// for: the argument list of gt_linear_fwd_grouped / gt_linear_bwd_grouped, in its order (`LinBwd c{x_dtype, ..., stream};` fills it, every
// option off), then the options the variant entry points add.  The public entry points fill a record and call lin_fwd / lin_bwd; so do
// `compute` is a gt_compute value: lin_fwd / lin_bwd normalise it ONCE, on their own copy of the record -- GT_COMPUTE_F32_HIGH becomes
// GT_F32 with `high` set -- so every `compute == GT_F32` test of the dispatchers sees fp32 semantics and the permission to run three
// products travels with the call (into L32Args / L32DwArgs), never through a process-wide option.
// the library's own layers (layers.hip, model.hip), which never go through the set-before-the-call entry points (gt_linear_set_rows*,
// gt_linear_bwd_bnstats, gt_linear_bwd_bcast: the outside ABI only).
#pragma once
#include "gt_common.h"

// forward: output row m is stored at row rows[m] of y; backward: row m of dY is row rows[m] of dy; -1 = no such row (gt_linear_set_rows)
// forward only: + a LayerNorm of the stored output row in the same epilogue when ln_out is set (gt_linear_set_rows_layernorm)
// forward only: + a row-gathered fp32 addend, y[rows[m]] = T(gemm row m + add_table[add_idx[m]][0..N)) with the sum in fp32 (before the
// LayerNorm above; add_idx[m] < 0: nothing added) when add_table is set (gt_linear_set_rows_add); needs `rows`
struct LinRowMap {
  const int32_t* rows;
  const float *ln_w, *ln_b;
  void* ln_out;
  float *ln_mean, *ln_rstd, ln_eps;
  const float* add_table;
  const int32_t* add_idx;
  int64_t add_ld;
};
struct LinFwd {
  int x_dtype, y_dtype, compute;
  const void* x;
  const float *weight, *bias;
  void* y;
  int64_t M, N, K, ldx, ldy;
  int groups;
  int64_t x_group_stride, y_group_stride;
  int act;
  float dropout_p;
  uint64_t seed;
  hipStream_t stream;
  void* gout;       // act == 2: receives the backward's multiplier (gt_linear_fwd_gelu), or null
  const void* x2;   // contraction columns [x_split, K) of the row operand come from this matrix, pitch ldx2 (gt_linear_fwd_cat2)
  int64_t x_split, ldx2;
  LinRowMap map;
  bool high;        // three bf16 products per fp32 product allowed (set by lin_fwd from compute == GT_COMPUTE_F32_HIGH, which it turns into GT_F32)
};
struct LinBwd {
  int x_dtype, y_dtype, compute;
  const void* x;
  const float* weight;
  const void *dy, *y_for_mask, *dx_add1, *dx_add2;
  void* dx;
  float *dweight, *dbias;
  int64_t M, N, K, ldx, ldy;
  int groups;
  int64_t x_group_stride, y_group_stride;
  float dropout_p;
  void* workspace;
  size_t workspace_bytes;
  hipStream_t stream;
  bool mul_mask;           // y_for_mask is a MULTIPLIER (gt_linear_bwd_mul), not a forward output
  bool fork_dw_only;       // dW-only call that may still go to the overlap stream (gt_linear_bwd_dw_forked)
  bool gate_out;           // y_for_mask [M][ldx] gates the dX OUTPUT (gt_linear_bwd_gate_out), dY is used as it is
  const float* weight_t;   // W^T [K][N] prepared by the caller (gt_linear_bwd_wt): no transpose launch
  // BatchNorm-backward statistics to accumulate in the dX epilogue (gt_linear_bwd_bnstats); bn_part == null: none
  const float *bn_x, *bn_mean, *bn_rstd, *bn_w, *bn_b;
  float* bn_part;
  int64_t bn_ldx;
  int bn_relu;
  int bn_nparts;           // partial rows bn_part was sized for: names the dX kernel (wide_dx); 0 = as the option says at the call
  const float* bcast;      // dX += bcast[bcast_idx[row]] (gt_linear_bwd_bcast)
  const int32_t* bcast_idx;
  // the row operand / the dX as two matrices side by side (gt_linear_bwd_cat2): columns [x_split, K) in x2 / dx2, pitch ldx2
  const void* x2;
  void* dx2;
  int64_t x_split, ldx2;
  LinRowMap map;
  bool high;               // as LinFwd::high (set by lin_bwd)
};
__attribute__((visibility("hidden"))) int lin_fwd(const LinFwd& f);
__attribute__((visibility("hidden"))) int lin_bwd(const LinBwd& c);
