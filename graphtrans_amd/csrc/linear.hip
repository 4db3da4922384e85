// linear.hip — nn.Linear forward / backward on the CDNA4 matrix cores for the skinny GEMMs of the
// GraphTrans hot path (M = nodes or tokens ~ 3e4, K and N in 128..600), with the surrounding
// elementwise work fused in.
//
// Reference call sites (paths under /root/reference): GCNConv.linear modules/conv.py:44,51; GIN mlp
// conv.py:18-20; virtual-node MLP modules/gnn_module.py:161-170; gnn2transformer
// models/gnn_transformer.py:69-70,92; nn.TransformerEncoderLayer in_proj / out_proj / linear1 (+act
// +dropout) / linear2 modules/transformer_encoder.py:28-32 — cuBLAS GEMM + bias + relu + dropout
// as separate launches in the reference; the first profile here (profiles/r01a) showed the library
// GEMMs at 2-4 % of the MFMA rate on these shapes and ~450 elementwise/cast/reduce launches per step.
//
//   fwd : Y[M][N]  = act(X[M][K] W[N][K]^T + b) (* dropout)           k_linear_fwd   ("NT")
//   dX  : dX[M][K] = dZ[M][N] W[N][K],  dZ = dY * 1[Y>0] * inv_keep   k_linear_dx    ("NN")
//   dW  : dW[N][K] = dZ^T X,  db[N] = colsum(dZ)                      k_linear_dw    ("TN", split over M)
// W is always the fp32 master weight (converted while staging: no cast pass); X / Y storage fp32 or
// bf16; compute type bf16 (v_mfma_f32_16x16x32_bf16) or fp32 (v_mfma_f32_16x16x4_f32, exact).
// Orientation: every lane owns an output ROW index as its MFMA column (n = lane & 15) and 4
// consecutive output columns as accumulator registers -> 8/16-byte stores, float4 bias loads.
#include <mutex>

#include "gt_common.h"
#include "linear_call.h"
#include "mfma_frag.h"

namespace {
using namespace gtf;

constexpr int LT = 256;  // threads
constexpr int BN = 128;

struct LinArgs {
  const void* a;      // fwd: X[M][K]; dx: dY[M][N]; dw: dY[M][N]
  const float* w;     // W[N][K] fp32
  const float* bias;  // [N] or null
  const void* x;      // dw: X[M][K]
  const void* ymask;  // dx/dw: forward output Y[M][N] when the forward fused relu(/dropout): dZ = dY*(Y>0)*inv_keep
  const void* add1;   // dx: optional addends [M][K] (storage type of dX): dX = dZ W + add1 + add2
  const void* add2;
  void* out;          // fwd: Y; dx: dX; dw: partial [splits][N][K] fp32
  float* dbpart;      // dw: [splits][N]
  int64_t M, N, K;
  int64_t ldy;        // row stride (elements) of Y / dY / ymask; >= N
  int64_t ldx;        // row stride (elements) of X / dX / the dX addends; >= K
  int act;            // 0 none, 1 relu, 2 gelu (erf)
  void* gout;         // fwd, act == 2: [M][ldy] (storage type of Y) receives d act/dz * dropout scale, the backward's multiplier; or null
  float inv_keep;     // 1/(1-p)
  uint32_t thr, s0, s1;
  int splits;
  int ntiles;           // fwd / dx: column tiles per row tile; dw: output tiles per M-split (see tile_of_block)
  int ntx;              // dw: tiles along N
  int64_t m_per_split;
  int64_t n_per_split;  // dx: contraction range per blockIdx.z when splits > 1 (partials [splits][M][K] fp32 in `out`)
  // grouped launch (blockIdx.y = group g, e.g. the towers of PNAConv): element offsets added per group
  int64_t g_x, g_y, g_w, g_b;   // X / dX / addends ; Y / dY / ymask ; W [N][K] ; bias [N]
  int64_t g_part;               // dw: floats between the groups' partial buffers (dW partials + db partials)
};

template <typename TA>
__device__ __forceinline__ const void* goff(const void* p, int64_t elems) {
  return p ? static_cast<const void*>(static_cast<const TA*>(p) + elems) : nullptr;
}

__device__ __forceinline__ uint32_t lin_hash(uint32_t s0, uint32_t s1, uint32_t row, uint32_t col) {
  uint32_t x = (row * 0x9E3779B1u + s0) ^ (col * 0x85EBCA77u + s1);
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

template <typename TC>
struct Tile {
  static constexpr int BK = 32;
  static constexpr int PAD = sizeof(TC) == 2 ? 8 : 4;   // 16 B row pad
  static constexpr int LD = BK + PAD;
};

// ---- register-staged tile loader (global -> registers -> LDS), 16-byte chunks -------------------
// load() issues every global load of the tile (and of the optional dZ mask tile) before anything
// consumes them; store() converts to the compute type and writes LDS.  Splitting the two lets the
// next stage's loads fly while the current stage's MFMAs run (T14 "issue early / write late").
template <typename TS, typename TC, int ROWS, int COLS, int LDS_LD, bool MASK>
struct Loader {
  static constexpr int EPC = 16 / sizeof(TS);  // elements per 16-byte chunk
  static constexpr int CH = COLS / EPC;
  static constexpr int NIT = ROWS * CH / LT;
  static_assert(ROWS * CH % LT == 0, "tile must be a multiple of the block's chunk count");
  uint4 v[NIT];
  uint4 m[MASK ? NIT : 1];
  int off[NIT];  // element offset of this thread's chunks relative to the tile origin (r * ld + cc)

  __device__ __forceinline__ void init(int64_t ld) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = threadIdx.x + i * LT;
      off[i] = (c / CH) * (int)ld + (c % CH) * EPC;
    }
  }

  // origin = address of tile element (0,0); rows_rem / cols_rem = valid extent from the origin
  __device__ __forceinline__ void load(const TS* origin, int64_t rows_rem, int64_t cols_rem, const TS* mask_origin) {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = threadIdx.x + i * LT;
      const int r = c / CH, cc = (c % CH) * EPC;
      const bool ok = r < rows_rem && cc < cols_rem;
      v[i] = ok ? *reinterpret_cast<const uint4*>(origin + off[i]) : make_uint4(0, 0, 0, 0);
      if constexpr (MASK)
        m[i] = (ok && mask_origin) ? *reinterpret_cast<const uint4*>(mask_origin + off[i]) : make_uint4(0, 0, 0, 0);
    }
  }

  __device__ __forceinline__ void store(TC* lds, bool has_mask, float inv_keep) const {
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = threadIdx.x + i * LT;
      const int r = c / CH, cc = (c % CH) * EPC;
      float f[EPC];
      if constexpr (sizeof(TS) == 4) {
        f[0] = __uint_as_float(v[i].x); f[1] = __uint_as_float(v[i].y);
        f[2] = __uint_as_float(v[i].z); f[3] = __uint_as_float(v[i].w);
      } else {
        const uint32_t u[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          f[2 * q] = __uint_as_float(u[q] << 16);
          f[2 * q + 1] = __uint_as_float(u[q] & 0xffff0000u);
        }
      }
      if constexpr (MASK) {
        if (has_mask) {
          float y[EPC];
          if constexpr (sizeof(TS) == 4) {
            y[0] = __uint_as_float(m[i].x); y[1] = __uint_as_float(m[i].y);
            y[2] = __uint_as_float(m[i].z); y[3] = __uint_as_float(m[i].w);
          } else {
            const uint32_t u[4] = {m[i].x, m[i].y, m[i].z, m[i].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              y[2 * q] = __uint_as_float(u[q] << 16);
              y[2 * q + 1] = __uint_as_float(u[q] & 0xffff0000u);
            }
          }
#pragma unroll
          for (int e = 0; e < EPC; ++e) f[e] = gt_gate(f[e], y[e], inv_keep);
        }
      }
      TC* dst = lds + r * LDS_LD + cc;
      if constexpr (sizeof(TC) == 4) {
#pragma unroll
        for (int e = 0; e < EPC; e += 4) *reinterpret_cast<float4*>(dst + e) = make_float4(f[e], f[e + 1], f[e + 2], f[e + 3]);
      } else if constexpr (sizeof(TS) == 2) {
        // bf16 -> bf16 with no mask is a plain copy; with a mask the values were re-rounded above
        if (!MASK || !has_mask) {
          *reinterpret_cast<uint4*>(dst) = v[i];  // bf16 -> bf16: plain copy
        } else {
          uint4 o;
          o.x = gt_pack_bf16(f[0], f[1]);
          o.y = gt_pack_bf16(f[2], f[3]);
          o.z = gt_pack_bf16(f[4], f[5]);
          o.w = gt_pack_bf16(f[6], f[7]);
          *reinterpret_cast<uint4*>(dst) = o;
        }
      } else {
        uint2 o;
        o.x = gt_pack_bf16(f[0], f[1]);
        o.y = gt_pack_bf16(f[2], f[3]);
        *reinterpret_cast<uint2*>(dst) = o;
      }
    }
  }
};

// XCD-aware tile order for the row-parallel kernels: workgroup b runs on XCD b % 8 (each XCD has its
// own L2).  The NT column blocks of one row tile read the SAME activation rows, so they get ids that
// differ by 8 (same XCD, dispatched within 8*NT ids of each other): the rows cross the fabric once
// instead of NT times (PMC on the 300x300 GCN linears: 115 MB fetched for 38 MB of activations before).
// 1-D grid of 8*ceil(MT/8)*NT blocks; a different hardware mapping only costs the locality.
__device__ __forceinline__ void tile_of_block(int nt, int64_t& mt, int& ntile) {
  const int64_t b = blockIdx.x;
  const int64_t group = b / (8 * nt);
  const int r = (int)(b % (8 * nt));
  ntile = r / 8;
  mt = group * 8 + r % 8;
}

// Per-wave epilogue patch: 16 output rows x 64 output columns of fp32 staged through LDS so that the
// global stores are whole 256-byte row segments (the MFMA accumulator layout alone gives 32 B).
constexpr int PATCH_LD = 64 + 4;
constexpr int PATCH_FLOATS = 16 * PATCH_LD;

template <typename TO>
__device__ __forceinline__ void store_chunk(TO* p, float4 v) { gt_store4<TO>(p, v); }

// bias[col..col+3]; the last chunk of an N that is not a multiple of 4 must not read past the array
__device__ __forceinline__ float4 bias_chunk(const float* bias, int64_t col, int64_t N) {
  if (col + 4 <= N) return *reinterpret_cast<const float4*>(bias + col);
  float4 b = gt_zero4();
  if (col < N) b.x = bias[col];
  if (col + 1 < N) b.y = bias[col + 1];
  if (col + 2 < N) b.z = bias[col + 2];
  return b;
}

#include "linear32.h"
#include "linear3x.h"
#include "linear3r.h"
#include "linear1.h"
#include "linear2.h"
#include "linear_small.h"
#include "linear_heads.h"
#include "linear_dw16.h"

// ------------------------------------------------------------------------------------------------
// forward: Y = act(X W^T + b) [dropout]
// MFMA rows = output columns n (W rows), MFMA cols = output rows m (X rows).
// ------------------------------------------------------------------------------------------------
template <typename TX, typename TY, typename TC, int BMT>
__global__ void __launch_bounds__(LT) k_linear_fwd(LinArgs a) {
  constexpr int BK = Tile<TC>::BK, LD = Tile<TC>::LD;
  constexpr int BM = BMT, MI = BMT / 32;  // rows per block, m16-tiles per wave
  constexpr int TILE_ELEMS = (BM + BN) * LD;
  constexpr int PATCH_ELEMS = (int)(4 * PATCH_FLOATS * sizeof(float) / sizeof(TC));
  constexpr int LDS_ELEMS = 2 * TILE_ELEMS > PATCH_ELEMS ? 2 * TILE_ELEMS : PATCH_ELEMS;  // the epilogue patches reuse the tiles
  __shared__ __attribute__((aligned(16))) TC smem[LDS_ELEMS];
  TC* sX = smem;
  TC* sW = smem + BM * LD;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int wm = wid & 1, wn = wid >> 1;  // wave tile: rows wm*64.., cols wn*64..
  int64_t mt_;
  int nt_;
  tile_of_block(a.ntiles, mt_, nt_);
  const int64_t m0 = mt_ * BM, n0 = (int64_t)nt_ * BN;
  if (m0 >= a.M) return;
  if (blockIdx.y) {
    const int64_t grp = blockIdx.y;
    a.a = goff<TX>(a.a, grp * a.g_x);
    a.w += grp * a.g_w;
    if (a.bias) a.bias += grp * a.g_b;
    a.out = const_cast<void*>(goff<TY>(a.out, grp * a.g_y));
  }
  const TX* X = reinterpret_cast<const TX*>(a.a);
  f32x4 acc[4][MI];  // [n tile j][m tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  Loader<TX, TC, BM, BK, LD, false> lx;
  Loader<float, TC, BN, BK, LD, false> lw;
  const int64_t Mx = a.M - m0, Nw = a.N - n0;
  const TX* xo = X + m0 * a.ldx;
  const float* wo = a.w + n0 * a.K;
  lx.init(a.ldx);
  lw.init(a.K);
  lx.load(xo, Mx, a.K, nullptr);
  lw.load(wo, Nw, a.K, nullptr);
  auto compute = [&](const TC* cX, const TC* cW) {
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      Frag<TC> fx[MI], fw[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) fx[i] = frag_load(cX + (wm * (BM / 2) + i * 16 + n) * LD + kk * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) fw[j] = frag_load(cW + (wn * 64 + j * 16 + n) * LD + kk * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[j][i] = mma(fw[j], fx[i], acc[j][i]);
    }
  };
  // two LDS stages, ONE barrier per k-step: stage s+1 is written while stage s is being multiplied (the
  // barrier that ended step s-1 freed that buffer); the global loads of stage s+2 are issued before the MFMAs
  // of stage s and land in registers during them
  lx.store(sX, false, 1.f);
  lw.store(sW, false, 1.f);
  if (BK < a.K) {
    lx.load(xo + BK, Mx, a.K - BK, nullptr);
    lw.load(wo + BK, Nw, a.K - BK, nullptr);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t k0 = 0; k0 < a.K; k0 += BK, cur ^= 1) {
    if (k0 + BK < a.K) {
      lx.store(sX + (cur ^ 1) * TILE_ELEMS, false, 1.f);
      lw.store(sW + (cur ^ 1) * TILE_ELEMS, false, 1.f);
      if (k0 + 2 * BK < a.K) {
        lx.load(xo + k0 + 2 * BK, Mx, a.K - k0 - 2 * BK, nullptr);
        lw.load(wo + k0 + 2 * BK, Nw, a.K - k0 - 2 * BK, nullptr);
      }
    }
    compute(sX + cur * TILE_ELEMS, sW + cur * TILE_ELEMS);
    __syncthreads();
  }
  // epilogue: acc[j][i][r] = C[col n0+wn*64+j*16+g*4+r][row m0+wm*64+i*16+n] -> patch[row n][col ...]
  float* patch = reinterpret_cast<float*>(smem) + wid * PATCH_FLOATS;
  TY* Y = reinterpret_cast<TY*>(a.out);
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(patch + n * PATCH_LD + j * 16 + g * 4) =
          make_float4(acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]);
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = lane + q * 64;       // 256 float4 chunks: row = c / 16, col4 = c % 16
      const int r = c >> 4, c4 = (c & 15) * 4;
      const int64_t m = m0 + wm * (BM / 2) + i * 16 + r;
      const int64_t col = n0 + wn * 64 + c4;
      if (m < a.M && col < a.N) {
        float4 v = *reinterpret_cast<const float4*>(patch + r * PATCH_LD + c4);
        if (a.bias) v = gt_add4(v, bias_chunk(a.bias, col, a.N));
        float4 gm = gt_zero4();
        float* vv = reinterpret_cast<float*>(&v);
        float* gg = reinterpret_cast<float*>(&gm);
        if (a.act == 1) v = gt_relu4(v);
        else if (a.act == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) gt_gelu(vv[e], vv[e], gg[e]);
        }
        if (a.thr) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool keep = lin_hash(a.s0, a.s1, (uint32_t)m, (uint32_t)(col + e)) >= a.thr;
            vv[e] = keep ? vv[e] * a.inv_keep : 0.f;
            gg[e] = keep ? gg[e] * a.inv_keep : 0.f;
          }
        }
        store_chunk<TY>(Y + m * a.ldy + col, v);
        if (a.act == 2 && a.gout) store_chunk<TY>(reinterpret_cast<TY*>(a.gout) + m * a.ldy + col, gm);
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ------------------------------------------------------------------------------------------------
// dX[M][K] = dZ[M][N] W[N][K]      (contraction over n)
// MFMA rows = output columns k (A operand = W^T via transposed LDS read), MFMA cols = rows m.
// ------------------------------------------------------------------------------------------------
template <typename TY, typename TX, typename TC, int BMT>
__global__ void __launch_bounds__(LT) k_linear_dx(LinArgs a) {
  constexpr int BM = BMT, MI = BMT / 32;
  constexpr int BKc = Tile<TC>::BK;            // n-slots per stage
  constexpr int LDZ = Tile<TC>::LD;            // dZ tile [BM][BKc]
  constexpr int LDW = BN + Tile<TC>::PAD;      // W tile [BKc n][BN k]
  constexpr int TILE_ELEMS = BM * LDZ + BKc * LDW;
  constexpr int PATCH_ELEMS = (int)(4 * PATCH_FLOATS * sizeof(float) / sizeof(TC));
  constexpr int LDS_ELEMS = 2 * TILE_ELEMS > PATCH_ELEMS ? 2 * TILE_ELEMS : PATCH_ELEMS;  // two stages (see k_linear_fwd)
  __shared__ __attribute__((aligned(16))) TC smem[LDS_ELEMS];
  TC* sZ = smem;
  TC* sW = smem + BM * LDZ;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int wm = wid & 1, wk = wid >> 1;
  int64_t mt_;
  int nt_;
  tile_of_block(a.ntiles, mt_, nt_);
  const int64_t m0 = mt_ * BM, kk0 = (int64_t)nt_ * BN;  // output column tile (k)
  if (m0 >= a.M) return;
  if (blockIdx.y) {
    const int64_t grp = blockIdx.y;
    a.a = goff<TY>(a.a, grp * a.g_y);
    a.ymask = goff<TY>(a.ymask, grp * a.g_y);
    a.w += grp * a.g_w;
    a.add1 = goff<TX>(a.add1, grp * a.g_x);
    a.add2 = goff<TX>(a.add2, grp * a.g_x);
    a.out = const_cast<void*>(goff<TX>(a.out, grp * a.g_x));
  }
  const TY* dY = reinterpret_cast<const TY*>(a.a);
  const TY* Ym = reinterpret_cast<const TY*>(a.ymask);
  const bool has_mask = Ym != nullptr;
  f32x4 acc[4][MI];  // [k tile j][m tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < MI; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  Loader<TY, TC, BM, BKc, LDZ, true> lz;
  Loader<float, TC, BKc, BN, LDW, false> lw;
  const TY* zo = dY + m0 * a.ldy;
  const TY* mo = has_mask ? Ym + m0 * a.ldy : nullptr;
  const float* wo = a.w + kk0;
  // contraction range of this block (whole N unless the launch splits it over blockIdx.z)
  const int64_t cb = a.splits > 1 ? (int64_t)blockIdx.z * a.n_per_split : 0;
  const int64_t ce = a.splits > 1 ? (cb + a.n_per_split < a.N ? cb + a.n_per_split : a.N) : a.N;
  lz.init(a.ldy);
  lw.init(a.K);
  if (cb < ce) {
    lz.load(zo + cb, a.M - m0, ce - cb, has_mask ? mo + cb : nullptr);
    lw.load(wo + cb * a.K, ce - cb, a.K - kk0, nullptr);
  }
  auto load_stage = [&](int64_t c1) {
    lz.load(zo + c1, a.M - m0, ce - c1, has_mask ? mo + c1 : nullptr);
    lw.load(wo + c1 * a.K, ce - c1, a.K - kk0, nullptr);
  };
  if (cb < ce) {
    lz.store(sZ, has_mask, a.inv_keep);
    lw.store(sW, false, 1.f);
    if (cb + BKc < ce) load_stage(cb + BKc);
  }
  __syncthreads();
  int cur = 0;
  for (int64_t c0 = cb; c0 < ce; c0 += BKc, cur ^= 1) {
    if (c0 + BKc < ce) {
      lz.store(sZ + (cur ^ 1) * TILE_ELEMS, has_mask, a.inv_keep);
      lw.store(sW + (cur ^ 1) * TILE_ELEMS, false, 1.f);
      if (c0 + 2 * BKc < ce) load_stage(c0 + 2 * BKc);
    }
    const TC* cZ = sZ + cur * TILE_ELEMS;
    const TC* cW = sW + cur * TILE_ELEMS;
#pragma unroll
    for (int s = 0; s < BKc / 32; ++s) {
      Frag<TC> fz[MI], fw[4];
#pragma unroll
      for (int i = 0; i < MI; ++i) fz[i] = frag_load(cZ + (wm * (BM / 2) + i * 16 + n) * LDZ + s * 32 + g * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) fw[j] = frag_load_tr(cW, LDW, s * 32, wk * 64 + j * 16, n, g);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MI; ++i) acc[j][i] = mma(fw[j], fz[i], acc[j][i]);
    }
    __syncthreads();
  }
  float* patch = reinterpret_cast<float*>(smem) + wid * PATCH_FLOATS;
  TX* dX = reinterpret_cast<TX*>(a.out);
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<float4*>(patch + n * PATCH_LD + j * 16 + g * 4) =
          make_float4(acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]);
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = lane + q * 64;
      const int r = c >> 4, c4 = (c & 15) * 4;
      const int64_t m = m0 + wm * (BM / 2) + i * 16 + r;
      const int64_t col = kk0 + wk * 64 + c4;
      if (m < a.M && col < a.K && a.splits > 1) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + ((int64_t)blockIdx.z * a.M + m) * a.K + col) =
            *reinterpret_cast<const float4*>(patch + r * PATCH_LD + c4);
      } else if (m < a.M && col < a.K) {
        float4 v = *reinterpret_cast<const float4*>(patch + r * PATCH_LD + c4);
        if (a.add1) v = gt_add4(v, gt_load4<TX>(reinterpret_cast<const TX*>(a.add1) + m * a.ldx + col));
        if (a.add2) v = gt_add4(v, gt_load4<TX>(reinterpret_cast<const TX*>(a.add2) + m * a.ldx + col));
        store_chunk<TX>(dX + m * a.ldx + col, v);
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ------------------------------------------------------------------------------------------------
// dW[N][K] = dZ^T X, db = colsum(dZ)      (contraction over m, split across blockIdx.z)
// MFMA rows = n (A = dZ^T via transposed LDS read), MFMA cols = k (B = X^T via transposed read).
// ------------------------------------------------------------------------------------------------
template <typename TY, typename TX, typename TC>
__global__ void __launch_bounds__(LT) k_linear_dw(LinArgs a) {
  constexpr int BMc = Tile<TC>::BK;            // m-slots per stage
  constexpr int LDZ = BN + Tile<TC>::PAD;      // dZ tile [BMc m][BN n]
  constexpr int LDX = BN + Tile<TC>::PAD;      // X tile  [BMc m][BN k]
  constexpr int TILE_ELEMS = BMc * (LDZ + LDX);
  constexpr int PATCH_ELEMS = (int)(4 * PATCH_FLOATS * sizeof(float) / sizeof(TC));
  constexpr int LDS_ELEMS = TILE_ELEMS > PATCH_ELEMS ? TILE_ELEMS : PATCH_ELEMS;
  __shared__ __attribute__((aligned(16))) TC smem[LDS_ELEMS];
  TC* sZ = smem;
  TC* sX = smem + BMc * LDZ;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  const int wn = wid & 1, wk = wid >> 1;
  // XCD-aware: the tiles of one M-split read the same dZ / X rows -> same XCD (see tile_of_block)
  int64_t split_;
  int tile_;
  tile_of_block(a.ntiles, split_, tile_);
  if (split_ >= a.splits) return;
  if (blockIdx.y) {
    const int64_t grp = blockIdx.y;
    a.a = goff<TY>(a.a, grp * a.g_y);
    a.ymask = goff<TY>(a.ymask, grp * a.g_y);
    a.x = goff<TX>(a.x, grp * a.g_x);
    a.out = static_cast<float*>(a.out) + grp * a.g_part;
    if (a.dbpart) a.dbpart += grp * a.g_part;
  }
  const int split = (int)split_;
  const int tx = tile_ % a.ntx, ty = tile_ / a.ntx;
  const int64_t n0 = (int64_t)tx * BN, k0 = (int64_t)ty * BN;
  const int64_t mb = (int64_t)split * a.m_per_split;
  const int64_t me = mb + a.m_per_split < a.M ? mb + a.m_per_split : a.M;
  const TY* dY = reinterpret_cast<const TY*>(a.a);
  const TY* Ym = reinterpret_cast<const TY*>(a.ymask);
  const bool has_mask = Ym != nullptr;
  const TX* X = reinterpret_cast<const TX*>(a.x);
  f32x4 acc[4][4];  // [n tile j][k tile i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;  // thread t < BN: column n0 + t
  Loader<TY, TC, BMc, BN, LDZ, true> lz;
  Loader<TX, TC, BMc, BN, LDX, false> lx;
  lz.init(a.ldy);
  lx.init(a.ldx);
  if (mb < me) {
    lz.load(dY + mb * a.ldy + n0, me - mb, a.N - n0, has_mask ? Ym + mb * a.ldy + n0 : nullptr);
    lx.load(X + mb * a.ldx + k0, me - mb, a.K - k0, nullptr);
  }
  // (single LDS stage here: a second one costs this kernel, with its 64 accumulator registers and 17 KB tiles,
  // more occupancy than the saved barrier returns -- measured 4-8 % slower)
  for (int64_t m0 = mb; m0 < me; m0 += BMc) {
    __syncthreads();
    lz.store(sZ, has_mask, a.inv_keep);
    lx.store(sX, false, 1.f);
    __syncthreads();
    if (m0 + BMc < me) {
      const int64_t m1 = m0 + BMc;
      lz.load(dY + m1 * a.ldy + n0, me - m1, a.N - n0, has_mask ? Ym + m1 * a.ldy + n0 : nullptr);
      lx.load(X + m1 * a.ldx + k0, me - m1, a.K - k0, nullptr);
    }
    if (ty == 0 && threadIdx.x < BN) {
#pragma unroll 8
      for (int r = 0; r < BMc; ++r) {
        const TC v = sZ[r * LDZ + threadIdx.x];
        if constexpr (sizeof(TC) == 2) dbacc += gt_bf16_to_f32((gt_bf16)v);
        else dbacc += (float)v;
      }
    }
#pragma unroll
    for (int s = 0; s < BMc / 32; ++s) {
      Frag<TC> fz[4], fx[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) fz[j] = frag_load_tr(sZ, LDZ, s * 32, wn * 64 + j * 16, n, g);
#pragma unroll
      for (int i = 0; i < 4; ++i) fx[i] = frag_load_tr(sX, LDX, s * 32, wk * 64 + i * 16, n, g);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = mma(fz[j], fx[i], acc[j][i]);
    }
  }
  __syncthreads();
  // acc[j][i][r] = C[row n-index wn*64+j*16+g*4+r][col k-index wk*64+i*16+n] -> patch[16 n rows][64 k cols]
  float* patch = reinterpret_cast<float*>(smem) + wid * PATCH_FLOATS;
  float* part = reinterpret_cast<float*>(a.out) + (int64_t)split * a.N * a.K;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) patch[(g * 4 + r) * PATCH_LD + i * 16 + n] = acc[j][i][r];
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = lane + q * 64;
      const int r = c >> 4, c4 = (c & 15) * 4;
      const int64_t row = n0 + wn * 64 + j * 16 + r;
      const int64_t col = k0 + wk * 64 + c4;
      if (row < a.N && col < a.K)
        *reinterpret_cast<float4*>(part + row * a.K + col) = *reinterpret_cast<const float4*>(patch + r * PATCH_LD + c4);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  if (ty == 0 && threadIdx.x < BN && n0 + threadIdx.x < a.N && a.dbpart)
    a.dbpart[(int64_t)split * a.N + n0 + threadIdx.x] = dbacc;
}

// out[i] = sum_s part[s][i]  (fixed order, 8 loads in flight).  One launch reduces two partial arrays:
// dW (len N*K -> out) and, when len2 > 0, db (len2 = N -> out2).
__global__ void __launch_bounds__(256) k_split_reduce(const float* __restrict__ part, int splits, int64_t len,
                                                      float* __restrict__ out, const float* __restrict__ part2, int64_t len2,
                                                      float* __restrict__ out2, int64_t g_part) {
  if (blockIdx.y) {   // grouped launch: the groups' partial buffers are g_part floats apart, outputs back to back
    part += blockIdx.y * g_part;
    out += blockIdx.y * len;
    if (part2) { part2 += blockIdx.y * g_part; out2 += blockIdx.y * len2; }
  }
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < len + len2; i0 += (int64_t)gridDim.x * 256) {
    const bool second = i0 >= len;
    const float* p = second ? part2 : part;
    const int64_t n = second ? len2 : len, i = second ? i0 - len : i0;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 8 <= splits; s += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += p[(int64_t)(s + u) * n + i];
    }
    for (; s < splits; ++s) acc[0] += p[(int64_t)s * n + i];
    (second ? out2 : out)[i] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
}

int check_lin(const char* fn, int x_dtype, int y_dtype, int compute, int64_t M, int64_t N, int64_t K, int64_t ldy) {
  if ((x_dtype != GT_F32 && x_dtype != GT_BF16) || (y_dtype != GT_F32 && y_dtype != GT_BF16) ||
      (compute != GT_F32 && compute != GT_BF16)) { gt_set_error("%s: bad dtype", fn); return GT_ERR_INVALID_ARG; }
  // exact-fp32 MFMA over mixed storage: fp32 x with bf16 y (gnn2transformer writing bf16 token rows; its backward reads
  // the bf16 token gradient) is supported; bf16 x with fp32 compute is not a combination of this path
  if (compute == GT_F32 && x_dtype != GT_F32) { gt_set_error("%s: fp32 compute needs fp32 x storage", fn); return GT_ERR_UNSUPPORTED; }
  if (M < 0 || N <= 0 || K <= 0) { gt_set_error("%s: bad sizes", fn); return GT_ERR_INVALID_ARG; }
  if (ldy < N) { gt_set_error("%s: ldy (%lld) < N (%lld)", fn, (long long)ldy, (long long)N); return GT_ERR_INVALID_ARG; }
  if (ldy % 4 != 0 || K % 4 != 0) { gt_set_error("%s: ldy (= N unless given) and K must be multiples of 4 (got %lld, %lld)", fn, (long long)ldy, (long long)K); return GT_ERR_UNSUPPORTED; }
  if ((x_dtype == GT_BF16 && K % 8 != 0) || (y_dtype == GT_BF16 && ldy % 8 != 0)) { gt_set_error("%s: bf16 storage needs K (x) / ldy (y) to be multiples of 8", fn); return GT_ERR_UNSUPPORTED; }
  return GT_OK;
}

void fill_drop(LinArgs& a, float dropout_p, uint64_t seed) {
  a.inv_keep = 1.0f / (1.0f - dropout_p);
  double thr = (double)dropout_p * 4294967296.0;
  a.thr = dropout_p > 0.f ? (uint32_t)(thr > 4294967295.0 ? 4294967295.0 : (thr < 1.0 ? 1.0 : thr)) : 0u;
  a.s0 = (uint32_t)seed;
  a.s1 = (uint32_t)(seed >> 32);
}

int dw_splits(int64_t M, int64_t N, int64_t K, int compute) {
  const int64_t bmc = compute == GT_BF16 ? 64 : 32;
  constexpr int target = 512;  // blocks per launch: partial traffic grows with it, parallelism too (flat 256..768 end to end)
  int64_t tiles = gt_cdiv(N, BN) * gt_cdiv(K, BN);
  int64_t s = target / tiles;
  int64_t maxs = gt_cdiv(M, bmc * 4);  // at least 4 stages per split
  if (s > maxs) s = maxs;
  if (s < 1) s = 1;
  if (s > 256) s = 256;
  return (int)s;
}

// dX with a long contraction (N >> M, K: the 5 x 5002-way prediction heads) has too few output tiles
// to fill the chip: split N over blockIdx.z into fp32 partials, reduced in fixed order.
int dx_splits(int64_t M, int64_t N, int64_t K, int bm) {
  const int64_t tiles = gt_cdiv(M, bm) * gt_cdiv(K, BN);
  if (tiles >= 128 || N < 2048) return 1;
  int64_t s = 512 / tiles;
  const int64_t maxs = N / 256;  // at least 4 stages of 64 per split
  if (s > maxs) s = maxs;
  if (s > 256) s = 256;
  return s < 2 ? 1 : (int)s;
}

// dispatch over (storage of the M-sized operands, compute type)
#define GT_LIN_DISPATCH(KERNEL, grid, args)                                                                        \
  do {                                                                                                             \
    if (compute == GT_F32 && t0 == GT_F32 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<float, float, float>), grid, dim3(LT), 0, stream, args); \
    else if (compute == GT_F32 && t0 == GT_F32) hipLaunchKernelGGL((KERNEL<float, gt_bf16, float>), grid, dim3(LT), 0, stream, args); \
    else if (compute == GT_F32) hipLaunchKernelGGL((KERNEL<gt_bf16, float, float>), grid, dim3(LT), 0, stream, args); \
    else if (t0 == GT_F32 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<float, float, gt_bf16>), grid, dim3(LT), 0, stream, args);   \
    else if (t0 == GT_F32 && t1 == GT_BF16) hipLaunchKernelGGL((KERNEL<float, gt_bf16, gt_bf16>), grid, dim3(LT), 0, stream, args); \
    else if (t0 == GT_BF16 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<gt_bf16, float, gt_bf16>), grid, dim3(LT), 0, stream, args); \
    else hipLaunchKernelGGL((KERNEL<gt_bf16, gt_bf16, gt_bf16>), grid, dim3(LT), 0, stream, args);                 \
  } while (0)

#define GT_LIN_DISPATCH_BM(KERNEL, BMV, grid, args)                                                                \
  do {                                                                                                             \
    if (compute == GT_F32 && t0 == GT_F32 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<float, float, float, BMV>), grid, dim3(LT), 0, stream, args); \
    else if (compute == GT_F32 && t0 == GT_F32) hipLaunchKernelGGL((KERNEL<float, gt_bf16, float, BMV>), grid, dim3(LT), 0, stream, args); \
    else if (compute == GT_F32) hipLaunchKernelGGL((KERNEL<gt_bf16, float, float, BMV>), grid, dim3(LT), 0, stream, args); \
    else if (t0 == GT_F32 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<float, float, gt_bf16, BMV>), grid, dim3(LT), 0, stream, args);   \
    else if (t0 == GT_F32 && t1 == GT_BF16) hipLaunchKernelGGL((KERNEL<float, gt_bf16, gt_bf16, BMV>), grid, dim3(LT), 0, stream, args); \
    else if (t0 == GT_BF16 && t1 == GT_F32) hipLaunchKernelGGL((KERNEL<gt_bf16, float, gt_bf16, BMV>), grid, dim3(LT), 0, stream, args); \
    else hipLaunchKernelGGL((KERNEL<gt_bf16, gt_bf16, gt_bf16, BMV>), grid, dim3(LT), 0, stream, args);            \
  } while (0)

// ---- optional overlap of the weight-gradient GEMMs (gt_overlap_dw_*): per host thread ------------
struct DwPending {
  uintptr_t lo, hi;   // workspace range a forked dW GEMM (partials + its reduce) still uses
  hipEvent_t ev;      // recorded on the side stream behind it
};
constexpr int DW_RING = 32;   // an encoder stage books 6 launches (4 dW GEMMs, 2 LayerNorm finishes), two stages are in flight
struct DwOverlap {
  bool active = false;
  hipStream_t main = nullptr, side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool urgent = false;       // the forks from here on are the last of the backward: the optimizer waits for them
  DwPending ring[DW_RING];   // forks since the last full join, oldest first (the side stream runs them in this order)
  int n = 0;
};
thread_local DwOverlap g_dw;

void dw_forked(const void* workspace, size_t bytes);
// main waits for the side stream; nothing is pending afterwards
void dw_join_all() {
  (void)hipEventRecord(g_dw.ev_join, g_dw.side);
  (void)hipStreamWaitEvent(g_dw.main, g_dw.ev_join, 0);
  g_dw.n = 0;
}
// main waits for the forked dW GEMMs whose workspace overlaps [p, p + bytes) -- and, the side stream being in order, for
// everything forked before them; later forks on other workspaces keep running
void dw_release(const void* p, size_t bytes) {
  if (!g_dw.active || !g_dw.n) return;
  const uintptr_t lo = (uintptr_t)p, hi = lo + bytes;
  int last = -1;
  for (int i = 0; i < g_dw.n; ++i)
    if (g_dw.ring[i].lo < hi && lo < g_dw.ring[i].hi) last = i;
  if (last < 0) return;
  (void)hipStreamWaitEvent(g_dw.main, g_dw.ring[last].ev, 0);
  // drop entries 0..last; their events rotate to the free end of the ring
  DwPending keep[DW_RING];
  int k = 0;
  for (int i = last + 1; i < g_dw.n; ++i) keep[k++] = g_dw.ring[i];
  const int kept = k;
  for (int i = 0; i <= last; ++i) keep[k++] = g_dw.ring[i];
  for (int i = g_dw.n; i < DW_RING; ++i) keep[k++] = g_dw.ring[i];
  for (int i = 0; i < DW_RING; ++i) g_dw.ring[i] = keep[i];
  g_dw.n = kept;
}
// called right after a dW GEMM (and its reduce) went to the side stream
void dw_forked(const void* workspace, size_t bytes) {
  if (g_dw.n == DW_RING) dw_join_all();
  DwPending& e = g_dw.ring[g_dw.n++];
  e.lo = (uintptr_t)workspace;
  e.hi = e.lo + bytes;
  (void)hipEventRecord(e.ev, g_dw.side);
}

// ---- deferred partial-sum reduces ----------------------------------------------------------------------------------------------
// Every weight-gradient GEMM ends in a fixed-order sum over its M-split partials (k_split_reduce), every LayerNorm backward in a column
// finish over its block partials: ~30 launches of 5-15 us per step that produce PARAMETER gradients only -- nothing before the
// optimizer / the gradient all-reduce reads them.  Inside a section (gt_defer_begin: the whole-model backward, csrc/model.hip) the
// producers put their partials into the section's arena (gt_defer_take) and queue the sum (gt_defer_push); gt_defer_flush runs all
// queued sums as ONE launch (k_defer_reduce: job list in the kernel arguments, same summation order as k_split_reduce -> same bits).
// The arena is never reused inside a section, so a flush may run on any stream that is ordered behind the producers.
struct DeferJob {
  const float *part, *part2;   // part[s * stride + i], s < nparts
  float *out, *out2;
  int64_t len, len2, stride, stride2;
  int64_t ostride;             // out[i * ostride] (1 = contiguous; the second array is always contiguous)
  int32_t nparts, block0;
};
constexpr int DEFER_MAX_JOBS = 44;   // 44 x 80 bytes of kernel arguments
struct DeferJobs {
  DeferJob j[DEFER_MAX_JOBS];
  int n;
};
struct DeferState {
  bool active = false;
  char* arena = nullptr;
  size_t cap = 0, used = 0;
  size_t max_take = 0;   // gt_defer_limit: requests above this many bytes are refused (0 = no limit)
  DeferJobs jobs{};
  int blocks = 0;
};
thread_local DeferState g_defer;

__global__ void __launch_bounds__(256) k_defer_reduce(DeferJobs J) {
  int ji = 0;
  for (int i = 1; i < J.n; ++i)
    if ((int)blockIdx.x >= J.j[i].block0) ji = i;
  const DeferJob& q = J.j[ji];
  const int nb = (ji + 1 < J.n ? J.j[ji + 1].block0 : (int)gridDim.x) - q.block0;
  for (int64_t i0 = (int64_t)((int)blockIdx.x - q.block0) * 256 + threadIdx.x; i0 < q.len + q.len2; i0 += (int64_t)nb * 256) {
    const bool second = i0 >= q.len;
    const float* p = second ? q.part2 : q.part;
    const int64_t st = second ? q.stride2 : q.stride, i = second ? i0 - q.len : i0;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 8 <= q.nparts; s += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) acc[u] += p[(int64_t)(s + u) * st + i];
    }
    for (; s < q.nparts; ++s) acc[0] += p[(int64_t)s * st + i];
    const float t = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    if (second) q.out2[i] = t;
    else q.out[i * q.ostride] = t;
  }
}

// the end of a weight-gradient GEMM: queue the sum over its partials (they live in the section's arena) or run it now
void dw_reduce(hipStream_t stream, bool deferred, const float* part, int splits, int64_t len, float* out, const float* part2, int64_t len2,
               float* out2) {
  if (deferred) {
    (void)gt_defer_push(part, splits, len, len, out, part2, len2, len2, out2);
    return;
  }
  const int rg = (int)(gt_cdiv(len + len2, 256) < 2048 ? gt_cdiv(len + len2, 256) : 2048);
  hipLaunchKernelGGL(k_split_reduce, dim3(rg, 1), dim3(256), 0, stream, part, splits, len, out, part2, len2, out2, (int64_t)0);
}
// its partial buffer: the open section's arena when it has room, else the caller's workspace
float* dw_part(float* ws_part, int splits, int64_t N, int64_t K, bool* deferred) {
  void* p = gt_defer_take((size_t)splits * (size_t)(N * K + N) * sizeof(float));
  *deferred = p != nullptr;
  return p ? (float*)p : ws_part;
}

int pick_bm(int64_t M, int64_t K = 0, bool fwd = false) {
  // 128-row tiles (half the blocks) measured 0.3-0.7 % slower end to end even for the 256-row GEMMs -- except the forward of a long
  // contraction over very many rows (the Erdos-Renyi stress' linear2, 131 k x 256 x 1024: every 64-row block re-stages the fp32
  // master weight, 2 GB of L2 reads for 335 MB of operands): 180 -> 144 us with 128 rows; its dX form gets slower (236 us)
  if (fwd && M >= 65536 && K >= 768) return 128;
  return 64;
}


// Short-M launches: a wave per tile pair when the tiles alone fill the chip, else the four waves of a block split the contraction
// of one tile pair (see small_combine in linear_small.h).
enum SmallKind { SMALL_FWD, SMALL_DX, SMALL_DW };
static inline void small_launch(SmallKind kind, int compute, int64_t tiles, int64_t contraction, hipStream_t stream, const SmallArgs& sa) {
  const bool sk = tiles <= 2048 && contraction >= 128;
  const unsigned blocks = (unsigned)(sk ? tiles : gt_cdiv(tiles, 4));
#define GT_SMALL_GO(KERNEL)                                                                                              \
  do {                                                                                                                    \
    if (compute == GT_F32) { if (sk) hipLaunchKernelGGL((KERNEL<float, 4>), dim3(blocks), dim3(256), 0, stream, sa);      \
                             else hipLaunchKernelGGL((KERNEL<float, 1>), dim3(blocks), dim3(256), 0, stream, sa); }       \
    else { if (sk) hipLaunchKernelGGL((KERNEL<gt_bf16, 4>), dim3(blocks), dim3(256), 0, stream, sa);                      \
           else hipLaunchKernelGGL((KERNEL<gt_bf16, 1>), dim3(blocks), dim3(256), 0, stream, sa); }                       \
  } while (0)
  if (kind == SMALL_FWD) GT_SMALL_GO(k_small_fwd);
  else if (kind == SMALL_DX) GT_SMALL_GO(k_small_dx);
  else GT_SMALL_GO(k_small_dw);
#undef GT_SMALL_GO
}


// ---- short-M path (linear_small.h): one wave per output tile pair, no LDS, no partials ---------------------------------------
// forward and dW of a short-M GEMM with a WIDE output (the 5 x 5002-way prediction heads, models/gnn_transformer.py:120-126: 256 rows
// x 25 010 columns): the one-wave-per-tile kernels have no limit on N (their work list just grows); only the dX form would walk N
// as its contraction and stays on the tiled split-N kernel
bool small_wide_ok(int x_dtype, int y_dtype, int64_t M, int64_t K, int64_t ldx, int64_t ldy, int groups) {
  return groups == 1 && x_dtype == GT_F32 && y_dtype == GT_F32 && M > 0 && M <= 512 && K <= 2048 && ldx % 4 == 0 && ldy % 4 == 0;
}
bool small_eligible(int x_dtype, int y_dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, int groups) {
  return groups == 1 && x_dtype == GT_F32 && y_dtype == GT_F32 && M > 0 && M <= 512 && N <= 2048 && K <= 2048 && ldx % 4 == 0 && ldy % 4 == 0;
}

// ---- exact-fp32 wide-tile path (linear32.h): the big-M GEMMs of the message-passing side --------------------------------
constexpr int64_t W32_MIN_M = 1024;   // below this the grid of 64-row blocks cannot fill the chip: 128-wide tiles + splits

bool w32_eligible(int compute, int x_dtype, int64_t M, int groups) {   // (compute: a gt_compute value, "high" is fp32)
  return gt_compute_base(compute) == GT_F32 && x_dtype == GT_F32 && groups == 1 && M >= W32_MIN_M;
}
// grouped launches of the bf16x6 kernel (k_lin3, blockIdx.y = group): fp32 rows in and out, 16-byte chunks of every row
bool g3_eligible(int compute, int x_dtype, int y_dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy) {
  return gt_compute_base(compute) == GT_F32 && x_dtype == GT_F32 && y_dtype == GT_F32 && M >= W32_MIN_M && N % 4 == 0 && K % 4 == 0 && ldx % 4 == 0 &&
         ldy % 4 == 0;
}

template <typename TA, typename TO, bool MASK, bool GELU = false, bool BNS = false>
void w32_launch_nt(int nt, dim3 grid, hipStream_t stream, const L32Args& a) {
  switch (nt) {
    case 19: hipLaunchKernelGGL((k_lin32<TA, TO, 19, MASK, GELU, BNS>), grid, dim3(256), 0, stream, a); break;
    case 16: hipLaunchKernelGGL((k_lin32<TA, TO, 16, MASK, GELU, BNS>), grid, dim3(256), 0, stream, a); break;
    case 12: hipLaunchKernelGGL((k_lin32<TA, TO, 12, MASK, GELU, BNS>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((k_lin32<TA, TO, 8, MASK, GELU, BNS>), grid, dim3(256), 0, stream, a); break;
  }
}

// out[M][Nout] = epilogue(A[M][Kc] W[Nout][Kc]^T): ta / to = storage of A / out
template <bool MASK>
void w32_launch(int ta, int to, hipStream_t stream, L32Args& a) {
  const int nt = w32_pick_nt(a.Nout);
  a.ncb = (int)gt_cdiv(gt_cdiv(a.Nout, 16), nt);
  dim3 grid((unsigned)(gt_cdiv(gt_cdiv(a.M, W32_BM), 8) * 8 * a.ncb));
  if constexpr (!MASK) {
    if (a.act == 2) {   // gelu epilogue: fp32 rows in and out only (w32_eligible_fwd)
      w32_launch_nt<float, float, false, true>(nt, grid, stream, a);
      return;
    }
  } else {
    if (a.bn_part) {    // BatchNorm-backward statistics in the dX epilogue: fp32 rows only (gt_linear_bwd_bnstats_ok)
      w32_launch_nt<float, float, true, false, true>(nt, grid, stream, a);
      return;
    }
  }
  if (ta == GT_F32 && to == GT_F32) w32_launch_nt<float, float, MASK>(nt, grid, stream, a);
  else if (ta == GT_F32) w32_launch_nt<float, gt_bf16, MASK>(nt, grid, stream, a);
  else if (to == GT_F32) w32_launch_nt<gt_bf16, float, MASK>(nt, grid, stream, a);
  else w32_launch_nt<gt_bf16, gt_bf16, MASK>(nt, grid, stream, a);
}

// M-splits of the wide-tile dW GEMM.  Alone on the chip it wants ~768 blocks (3 per CU is what its 48 KB of LDS admits; the
// dispatcher fills CUs greedily, 2 per CU leaves a third idle).  Forked onto the overlap stream (gt_overlap_dw_*) it shares
// the chip with the critical path: one block per CU leaves every CU room for the other streams' kernels (the 5-25 us kernels
// of the virtual-node chain ran 2-5 x longer beside an 800-block GEMM) and writes a third of the partials -- the GEMM
// itself takes longer, but nothing waits for it (Code2 +1.7 %, Molpcba +2 % end to end).
int w32_dw_splits(int64_t M, int nkb, int nnb, bool overlapped) {
  int64_t s = (overlapped ? 256 : 768) / ((int64_t)nkb * nnb);   // every split costs N*K*4 bytes of partials twice
  const int64_t maxs = gt_cdiv(M, 16 * 8);          // at least 8 stages per split
  if (s > maxs) s = maxs;
  if (s < 1) s = 1;
  if (s > 256) s = 256;
  return (int)s;
}

template <typename TY, typename TX>
void w32_launch_dw_nt(int nt, dim3 grid, hipStream_t stream, const L32DwArgs& a) {
  switch (nt) {
    case 19: hipLaunchKernelGGL((k_lin32_dw<TY, TX, 19, true>), grid, dim3(256), 0, stream, a); break;
    case 16: hipLaunchKernelGGL((k_lin32_dw<TY, TX, 16, true>), grid, dim3(256), 0, stream, a); break;
    case 12: hipLaunchKernelGGL((k_lin32_dw<TY, TX, 12, true>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((k_lin32_dw<TY, TX, 8, true>), grid, dim3(256), 0, stream, a); break;
  }
}


// ---- per-call requests of the outside ABI -----------------------------------------------------------------------------------------
// gt_linear_set_rows, gt_linear_set_rows_layernorm, gt_linear_set_rows_add, gt_linear_bwd_bnstats and gt_linear_bwd_bcast have no call of their own: what they
// ask for waits here, per host thread, for the next public gt_linear_fwd* / gt_linear_bwd* call, which moves it into its record
// (take_map / take_bwd: the only readers) -- only the request fields of this record are ever set.  The dispatchers below and the
// library's own layers never see it: they pass records.
thread_local LinBwd g_pending{};
// a forward call takes the row map, whatever its outcome, and leaves the backward's requests in place
LinRowMap take_map() {
  const LinRowMap m = g_pending.map;
  g_pending.map = LinRowMap{};
  return m;
}
// a backward call takes everything, whatever its outcome
void take_bwd(LinBwd& c) {
  const LinBwd& p = g_pending;
  c.map = p.map; c.bcast = p.bcast; c.bcast_idx = p.bcast_idx;
  c.bn_x = p.bn_x; c.bn_mean = p.bn_mean; c.bn_rstd = p.bn_rstd; c.bn_w = p.bn_w; c.bn_b = p.bn_b; c.bn_part = p.bn_part; c.bn_ldx = p.bn_ldx; c.bn_relu = p.bn_relu;
  g_pending = LinBwd{};
}
// errors raised inside the dispatchers keep the texts of the entry points they were split from
#define LIN_CHECK_ARG(fn, cond, msg) \
  do { if (!(cond)) { gt_set_error("%s: %s", fn, msg); return GT_ERR_INVALID_ARG; } } while (0)
#define LIN_DIMS(c) {(c).M, (c).N, (c).K, (c).x_dtype, (c).y_dtype, (c).compute}

// what the forward and the backward check alike (fn, what: the names their errors carry; min_ldx: K, or the split under cat2, whose first
// matrix holds columns [0, split))
int check_call(const char* fn, const char* what, int x_dtype, int y_dtype, int compute, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy,
               int64_t min_ldx, int groups, int64_t x_group_stride, int64_t y_group_stride) {
  LIN_CHECK_ARG(fn, groups >= 1 && groups <= 65535, "1..65535 groups");
  LIN_CHECK_ARG(fn, groups == 1 || (x_group_stride % (x_dtype == GT_BF16 ? 8 : 4) == 0 && y_group_stride % (y_dtype == GT_BF16 ? 8 : 4) == 0 && (N * K) % 4 == 0),
                "group strides must keep 16-byte alignment");
  const int rc = check_lin(what, x_dtype, y_dtype, compute, M, N, K, ldy);
  if (rc == GT_OK && (ldx < min_ldx || ldx % (x_dtype == GT_BF16 ? 8 : 4))) {
    gt_set_error("%s: ldx (%lld) must be >= K and a multiple of 16 bytes", what, (long long)ldx);
    return GT_ERR_UNSUPPORTED;
  }
  return rc;
}
bool rows_eligible(int compute, int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K) {
  return w32_eligible(compute, x_dtype, M, 1) && (y_dtype == GT_F32 || N % 8 == 0) && w3_lookup(weight, N, K, false) && w3_lookup(weight, N, K, true);
}

// ---- forward: one function per kernel family, in order of preference --------------------------------------------------------------
// Each either declines (false) or takes the call (true): it enqueues its launch, or sets rc to the error it met.
bool fwd_heads(const LinFwd& f, const LinArgs& a, int&) {   // the prediction heads (linear_heads.h)
  if (!heads_shape_ok(f.x_dtype, f.y_dtype, f.M, f.N, f.K, f.ldx, f.ldy, f.groups) || f.act != 0 || a.thr || f.gout) return false;
  hipStream_t stream = f.stream;
  HeadsArgs h{};
  h.x = (const float*)f.x; h.w = f.weight; h.bias = f.bias; h.out = (float*)f.y; h.M = f.M; h.N = f.N; h.ldx = f.ldx; h.ldy = f.ldy;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_heads_fwd", stream, LIN_DIMS(f));
  heads_launch_fwd(f.compute, stream, h);
  return true;
}
bool fwd_small(const LinFwd& f, const LinArgs& a, int&) {   // short M (linear_small.h), wide outputs included
  if (!small_eligible(f.x_dtype, f.y_dtype, f.M, f.N, f.K, f.ldx, f.ldy, f.groups) && !small_wide_ok(f.x_dtype, f.y_dtype, f.M, f.K, f.ldx, f.ldy, f.groups))
    return false;
  hipStream_t stream = f.stream;
  SmallArgs sa{};
  sa.x = (const float*)f.x; sa.w = f.weight; sa.bias = f.bias; sa.out = (float*)f.y; sa.M = f.M; sa.N = f.N; sa.K = f.K; sa.ldx = f.ldx; sa.ldy = f.ldy;
  sa.act = f.act; sa.gout = (float*)f.gout; sa.inv_keep = a.inv_keep; sa.thr = a.thr; sa.s0 = a.s0; sa.s1 = a.s1;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_small_fwd", stream, LIN_DIMS(f));
  small_launch(SMALL_FWD, f.compute, gt_cdiv(f.M, 16) * gt_cdiv(f.N, 32), f.K, stream, sa);
  return true;
}
// grouped big-M fp32 GEMMs whose group weights all have bound images (the towers of PNAConv): k_lin3 with blockIdx.y = group
bool fwd_grouped3(const LinFwd& f, const LinArgs& a, int&) {
  if (f.groups <= 1 || !g3_eligible(f.compute, f.x_dtype, f.y_dtype, f.M, f.N, f.K, f.ldx, f.ldy) || f.act == 2 || f.x2) return false;
  int64_t spacing = 0;
  const void* img = w3_lookup_grouped(f.weight, f.N, f.K, f.groups, false, &spacing);
  if (!img) return false;
  hipStream_t stream = f.stream;
  L32Args w{};
  w.a = f.x; w.bias = f.bias; w.out = f.y; w.M = f.M; w.Nout = f.N; w.Kc = f.K; w.lda = f.ldx; w.ldw = f.K; w.ldo = f.ldy;
  w.act = f.act; w.inv_keep = a.inv_keep; w.thr = a.thr; w.s0 = a.s0; w.s1 = a.s1;
  w.w3 = img; w.groups = f.groups; w.g_a = f.x_group_stride; w.g_o = f.y_group_stride; w.g_img = spacing; w.g_b = (int)f.N;
  w.high = f.high;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin3[fwd]", stream, LIN_DIMS(f));
  w3_launch<false>(f.x_dtype, f.y_dtype, stream, w);
  return true;
}
// big-M exact-fp32 compute: the bf16x6 kernels on a bound image of the weight (k_lin3r / k_lin3), else the exact-fp32 MFMA kernel (k_lin32)
bool fwd_wide(const LinFwd& f, const LinArgs& a, int& rc) {
  if (!w32_eligible(f.compute, f.x_dtype, f.M, f.groups) || (f.act == 2 && (f.x_dtype != GT_F32 || f.y_dtype != GT_F32))) return false;
  hipStream_t stream = f.stream;
  const auto fail = [&rc](const char* msg) { gt_set_error("%s", msg); rc = GT_ERR_UNSUPPORTED; return true; };
  L32Args w{};
  w.a = f.x; w.w = f.weight; w.bias = f.bias; w.out = f.y; w.M = f.M; w.Nout = f.N; w.Kc = f.K; w.lda = f.ldx; w.ldw = f.K; w.ldo = f.ldy;
  w.act = f.act; w.gout = f.gout; w.inv_keep = a.inv_keep; w.thr = a.thr; w.s0 = a.s0; w.s1 = a.s1;
  w.high = f.high;
  // a prepared bf16x3 image of this weight (gt_w3_bind): the fp32-accurate GEMM on the bf16 matrix pipe (linear3x.h);
  // bf16 rows need K % 8 (their 16-byte chunks are whole k-groups)
  w.w3 = (f.x_dtype == GT_F32 || f.K % 8 == 0) ? w3_lookup(f.weight, f.N, f.K, false) : nullptr;
  if (f.x2) {
    if (!w.w3 || f.x_dtype != GT_F32) return fail("gt_linear_fwd_cat2: needs a bound weight image and fp32 rows");
    w.a2 = f.x2; w.a_split = f.x_split; w.lda2 = f.ldx2;
  }
  if (f.map.rows) {
    if (!w.w3) return fail("gt_linear_set_rows: needs a bound weight image");
    w.out_rows = f.map.rows;
    if (f.map.ln_out) {
      if (w3_pick_nt(f.N) * 16 != f.N || f.act != 0 || a.thr || f.ldy != f.N)
        return fail("gt_linear_set_rows_layernorm: the row must fill one column block (ask gt_linear_rows_layernorm_ok)");
      w.ln_w = f.map.ln_w; w.ln_b = f.map.ln_b; w.ln_out = f.map.ln_out; w.ln_mean = f.map.ln_mean; w.ln_rstd = f.map.ln_rstd;
      w.ln_eps = f.map.ln_eps;
    }
    if (f.map.add_table) {
      if (f.act == 2) return fail("gt_linear_set_rows_add: not with the GELU epilogue");
      w.add_tab = f.map.add_table; w.add_idx = f.map.add_idx; w.add_ld = f.map.add_ld;
    }
  }
  const bool on_rows_kernel = w.w3 && w3r_ok(f.x_dtype, f.y_dtype, w);
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, on_rows_kernel ? "k_lin3r[fwd]" : (w.w3 ? "k_lin3[fwd]" : "k_lin32[fwd]"), stream, LIN_DIMS(f));
  if (on_rows_kernel) w3r_launch(stream, w);   // rows straight into fragments (linear3r.h)
  else if (w.w3) w3_launch<false>(f.x_dtype, f.y_dtype, stream, w);
  else w32_launch<false>(f.x_dtype, f.y_dtype, stream, w);
  return true;
}
// bf16 rows in and out with a bound fragment-order image of this weight (gt_w1_bind): the weight-stationary kernel (linear1.h)
bool fwd_bf16_image(const LinFwd& f, const LinArgs& a, int&) {
  if (f.x_dtype != GT_BF16 || f.y_dtype != GT_BF16 || f.compute != GT_BF16 || f.groups != 1 || f.act == 2 || f.M < W1_MIN_M) return false;
  const void* img = w1_lookup(f.weight, f.N, f.K, false);
  if (!img) return false;
  hipStream_t stream = f.stream;
  L1Args l{};
  l.a = (const gt_bf16*)f.x; l.img = (const unsigned char*)img; l.bias = f.bias; l.out = (gt_bf16*)f.y;
  l.M = f.M; l.lda = f.ldx; l.ldo = f.ldy; l.N = (int)f.N; l.K = (int)f.K; l.act = f.act;
  l.inv_keep = a.inv_keep; l.thr = a.thr; l.s0 = a.s0; l.s1 = a.s1;
  // many rows, or a contraction the registers cannot hold: both operands through the LDS ring (linear2.h)
  const bool ring = w2_take(l, w1_pick_ntw(f.N, f.K) != 0);
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, ring ? "k_lin2[fwd]" : "k_lin1[fwd]", stream, LIN_DIMS(f));
  return ring ? w2_launch(stream, l) : w1_launch(stream, l);   // (false: no launch, the tiled kernel runs it)
}
void fwd_tiled(const LinFwd& f, LinArgs a) {
  hipStream_t stream = f.stream;
  const int compute = f.compute, bm = pick_bm(f.M, f.K, true);
  a.ntiles = (int)gt_cdiv(f.N, BN);
  dim3 grid((unsigned)(gt_cdiv(gt_cdiv(f.M, bm), 8) * 8 * a.ntiles), (unsigned)f.groups);
  const int t0 = f.x_dtype, t1 = f.y_dtype;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_linear_fwd", stream, LIN_DIMS(f));
  if (bm == 64) GT_LIN_DISPATCH_BM(k_linear_fwd, 64, grid, a);
  else GT_LIN_DISPATCH_BM(k_linear_fwd, 128, grid, a);
}
}  // namespace

int lin_fwd(const LinFwd& f_) {
  const char* fn = "linear_fwd_impl";
  LinFwd f = f_;   // (the one place a forward's `compute` is normalised: linear_call.h)
  f.high = f.compute == GT_COMPUTE_F32_HIGH;
  f.compute = gt_compute_base(f.compute);
  LIN_CHECK_ARG(fn, !f.map.rows || (f.groups == 1 && rows_eligible(f.compute, f.x_dtype, f.y_dtype, f.weight, f.M, f.N, f.K)),
                "gt_linear_set_rows: this GEMM does not take a row map (ask gt_linear_rows_ok)");
  LIN_CHECK_ARG(fn, !f.map.add_table || (f.map.rows && f.map.add_idx && f.map.add_ld >= f.N && f.map.add_ld % 4 == 0 && ((uintptr_t)f.map.add_table & 15) == 0),
                "gt_linear_set_rows_add: the addend rides on a row map (gt_linear_set_rows*); fp32 table, 16-byte aligned, pitch >= N and a multiple of 4");
  int rc = check_call(fn, "gt_linear_fwd", f.x_dtype, f.y_dtype, f.compute, f.M, f.N, f.K, f.ldx, f.ldy, f.x2 ? f.x_split : f.K, f.groups,
                      f.x_group_stride, f.y_group_stride);
  if (rc) return rc;
  LIN_CHECK_ARG(fn, f.x && f.weight && f.y, "null buffer");
  LIN_CHECK_ARG(fn, f.dropout_p >= 0.f && f.dropout_p < 1.f, "dropout_p must be in [0,1)");
  if (f.M == 0) return GT_OK;
  GtProfScope prof__(GT_PROF_LINEAR, "gt_linear_fwd", f.stream, LIN_DIMS(f));
  LinArgs a{};
  a.a = f.x; a.w = f.weight; a.bias = f.bias; a.out = f.y; a.M = f.M; a.N = f.N; a.K = f.K; a.ldy = f.ldy; a.ldx = f.ldx; a.act = f.act; a.gout = f.gout;
  fill_drop(a, f.dropout_p, f.seed);
  a.g_x = f.x_group_stride; a.g_y = f.y_group_stride; a.g_w = f.N * f.K; a.g_b = f.N;
  if (!(fwd_heads(f, a, rc) || fwd_small(f, a, rc) || fwd_grouped3(f, a, rc) || fwd_wide(f, a, rc) || fwd_bf16_image(f, a, rc))) fwd_tiled(f, a);
  if (rc) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gt_set_error("%s: launch failed: %s", fn, hipGetErrorString(e)); return GT_ERR_LAUNCH; }
  return GT_OK;
}

extern "C" int gt_linear_fwd(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* bias, void* y, int64_t M,
                             int64_t N, int64_t K, int act, float dropout_p, uint64_t seed, gt_stream_t stream_) {
  return gt_linear_fwd_grouped(x_dtype, y_dtype, compute, x, weight, bias, y, M, N, K, K, N, 1, 0, 0, act, dropout_p, seed, stream_);
}

extern "C" int gt_linear_fwd_ld(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* bias, void* y, int64_t M,
                                int64_t N, int64_t K, int64_t ldy, int act, float dropout_p, uint64_t seed, gt_stream_t stream_) {
  return gt_linear_fwd_grouped(x_dtype, y_dtype, compute, x, weight, bias, y, M, N, K, K, ldy, 1, 0, 0, act, dropout_p, seed, stream_);
}

extern "C" int gt_linear_fwd_ld2(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* bias, void* y, int64_t M,
                                 int64_t N, int64_t K, int64_t ldx, int64_t ldy, int act, float dropout_p, uint64_t seed, gt_stream_t stream_) {
  return gt_linear_fwd_grouped(x_dtype, y_dtype, compute, x, weight, bias, y, M, N, K, ldx, ldy, 1, 0, 0, act, dropout_p, seed,
                               stream_);
}

extern "C" int gt_linear_fwd_grouped(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* bias, void* y, int64_t M,
                                     int64_t N, int64_t K, int64_t ldx, int64_t ldy, int groups, int64_t x_group_stride, int64_t y_group_stride,
                                     int act, float dropout_p, uint64_t seed, gt_stream_t stream_) {
  GT_CHECK_ARG(act == 0 || act == 1, "act must be 0 (none) or 1 (relu); gelu: gt_linear_fwd_gelu");
  GT_CHECK_ARG(dropout_p == 0.f || act == 1, "fused dropout requires a fused activation");
  LinFwd f{x_dtype, y_dtype, compute, x, weight, bias, y, M, N, K, ldx, ldy, groups, x_group_stride, y_group_stride, act, dropout_p, seed, (hipStream_t)stream_};
  f.map = take_map();
  return lin_fwd(f);
}

// Y = dropout(gelu(X W^T + b)); gmul = gelu'(z) * dropout scale: what gt_linear_bwd_mul takes in place of the ReLU path's forward output
extern "C" int gt_linear_fwd_gelu(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* bias, void* y, void* gmul,
                                  int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, float dropout_p, uint64_t seed, gt_stream_t stream_) {
  LinFwd f{x_dtype, y_dtype, compute, x, weight, bias, y, M, N, K, ldx, ldy, 1, 0, 0, 2, dropout_p, seed, (hipStream_t)stream_};
  f.gout = gmul;
  f.map = take_map();
  return lin_fwd(f);
}

extern "C" size_t gt_linear_bwd_workspace_bytes(int compute, int64_t M, int64_t N, int64_t K) {
  compute = gt_compute_base(compute);   // "high" sizes as fp32
  if (compute == GT_F32 && M >= W32_MIN_M) {   // wide-tile fp32 path: [dW / db partials | W^T for the dX GEMM]
    const int nt = w32_pick_nt(N);
    const int splits = w32_dw_splits(M, (int)gt_cdiv(K, 64), (int)gt_cdiv(gt_cdiv(N, 16), nt), false);   // the larger of the two configurations
    return (size_t)splits * (size_t)(N * K + N) * sizeof(float) + (size_t)N * K * sizeof(float) + 512;
  }
  const size_t dw = (size_t)dw_splits(M, N, K, compute) * (size_t)(N * K + N) * sizeof(float);
  const int dxs = dx_splits(M, N, K, pick_bm(M));
  size_t dx = dxs > 1 ? (size_t)dxs * M * K * sizeof(float) : 0;
  if (heads_shape_ok(GT_F32, GT_F32, M, N, K, 4, 4, 1) && heads_dx_workspace_bytes(M, N) > dx) dx = heads_dx_workspace_bytes(M, N);
  return (dw > dx ? dw : dx) + 256;  // the dx partials are consumed before dw reuses the space
}

extern "C" size_t gt_linear_bwd_grouped_workspace_bytes(int compute, int64_t M, int64_t N, int64_t K, int groups) {
  return (size_t)(groups < 1 ? 1 : groups) * gt_linear_bwd_workspace_bytes(compute, M, N, K);
}

// BatchNorm-backward statistics in the dX epilogue (include/graphtrans_hip.h): only the exact-fp32 wide-tile path does this
extern "C" int gt_linear_bwd_bnstats_ok(int compute, int x_dtype, int y_dtype, int64_t M) {
  return (w32_eligible(compute, x_dtype, M, 1) && x_dtype == GT_F32 && y_dtype == GT_F32) ? 1 : 0;
}
extern "C" int64_t gt_linear_bwd_bnstats_rows(int64_t M) { return gt_cdiv(M, W32_BM); }
// the register-row bf16x6 kernel (linear3r.h) takes a dX call with BatchNorm statistics in its epilogue: one partial row per 128-row block
// (only with gt_option_set("bnstats_rows_kernel", 1): measured slower than the separate partial pass -- Code2 74.0 k against 74.85 k
// graphs/s, round 5 -- and gt_linear_bwd_bnstats' documented partial layout is the exact kernel's 64-row tiles; kept as a tested
// alternative, tests/test_hip_options.py)
// (bns_rows_kernel_can: the shape question alone; the option is read where a caller SIZES the partial buffer -- a call that states the
// size it was given, LinBwd::bn_nparts, is run by the kernel that fills it and does not read the option again)
static bool bns_rows_kernel_can(int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy) {
  const void* img = w3_lookup(weight, N, K, true);
  if (!img || x_dtype != GT_F32 || y_dtype != GT_F32) return false;
  L32Args w{};
  w.w3 = img;
  w.M = M; w.Nout = K; w.Kc = N; w.lda = ldy; w.ldo = ldx;
  return w3r_ok(GT_F32, GT_F32, w);
}
static bool bns_on_rows_kernel(int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy) {
  return gt_opt(GT_OPT_BNSTATS_ROWS_KERNEL) && bns_rows_kernel_can(x_dtype, y_dtype, weight, M, N, K, ldx, ldy);
}
extern "C" int64_t gt_linear_bwd_bnstats_rows_for(int compute, int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K) {
  if (!gt_linear_bwd_bnstats_ok(compute, x_dtype, y_dtype, M)) return 0;
  return bns_on_rows_kernel(x_dtype, y_dtype, weight, M, N, K, K, N) ? gt_cdiv(M, 128) : gt_cdiv(M, W32_BM);
}
extern "C" int gt_linear_bwd_bnstats(const float* bn_x, int64_t ldx, const float* mean, const float* rstd, const float* w, const float* b, int relu,
                                     float* part) {
  GT_CHECK_ARG(bn_x && mean && rstd && w && b && part && ldx > 0, "null buffer");
  LinBwd& q = g_pending;
  q.bn_x = bn_x; q.bn_ldx = ldx; q.bn_mean = mean; q.bn_rstd = rstd; q.bn_w = w; q.bn_b = b; q.bn_relu = relu; q.bn_part = part;
  return GT_OK;
}

// a broadcast addend in the dX epilogue, dx[m] += rows[idx[m]] (include/graphtrans_hip.h): only the kernel with the rows in registers (linear3r.h)
extern "C" int gt_linear_bwd_bcast_ok(int compute, int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K) {
  if (!w32_eligible(compute, x_dtype, M, 1) || x_dtype != GT_F32 || y_dtype != GT_F32 || !w3_lookup(weight, N, K, true)) return 0;
  L32Args w{};
  w.w3 = w3_lookup(weight, N, K, true);
  w.M = M; w.Nout = K; w.Kc = N; w.lda = N; w.ldo = K;
  return w3r_ok(GT_F32, GT_F32, w) ? 1 : 0;
}
extern "C" int gt_linear_bwd_bcast(const float* rows, const int32_t* idx) {
  GT_CHECK_ARG((rows == nullptr) == (idx == nullptr), "rows and idx go together");
  g_pending.bcast = rows;
  g_pending.bcast_idx = idx;
  return GT_OK;
}

// out [K][N] = in [N][K]^T (fp32)
extern "C" int gt_transpose(const float* in, float* out, int64_t N, int64_t K, gt_stream_t stream_) {
  GT_CHECK_ARG(in && out && N > 0 && K > 0, "bad arguments");
  hipLaunchKernelGGL(k_transpose32, dim3((unsigned)gt_cdiv(K, 32), (unsigned)gt_cdiv(N, 32)), dim3(256), 0, (hipStream_t)stream_, in, out, N, K);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

namespace {
// ---- backward: one function per kernel family, in order of preference -------------------------------------------------------------
// What flows between them.  Each family either declines (it leaves the state as it is) or enqueues its launches and marks what it did.
struct BwdState {
  bool dx, dw;          // still to compute
  const void* ymask;    // the gate the GEMMs still to run apply to dY (gt_linear_bwd_gate_out: gone once the gated dX is out)
  int dx_splits;        // > 1: the tiled dX kernel left split-N partials in the workspace, a weight gradient must not fork behind it
  float inv_keep;       // of the gate; 0 = multiplier mode (gt_gate)
  size_t need;          // workspace bytes of the whole call
  int64_t g_part;       // floats between the groups' partial buffers
};

// dW is off the critical path of the backward (only the optimizer reads it): inside a gt_overlap_dw_begin/_end section the weight gradient
// of a call that also computes dX (or asks for it: gt_linear_bwd_dw_forked) runs on the side stream beside dX and whatever follows
// (not while the launch profiler brackets this call: its events sit on the caller's stream only).  `site` = the calling family's own
// condition.
bool dw_will_fork(const LinBwd& c, bool site) {
  return g_dw.active && c.stream == g_dw.main && (c.dx || c.fork_dw_only) && site && !(gt_prof_mask() & GT_PROF_LINEAR);
}
// -> the stream the weight gradient's launches go to, ordered behind everything queued on the caller's stream so far; when it is not
// the caller's, dw_forked(workspace, bytes) books them afterwards
hipStream_t dw_fork(const LinBwd& c, bool site) {
  if (!dw_will_fork(c, site)) return c.stream;
  (void)hipEventRecord(g_dw.ev_fork, g_dw.main);
  (void)hipStreamWaitEvent(g_dw.side, g_dw.ev_fork, 0);
  return g_dw.side;
}
void dw_book(const LinBwd& c, hipStream_t dw_stream) {
  if (dw_stream != c.stream) dw_forked(c.workspace, c.workspace_bytes);
}
void small_dw(const LinBwd& c, const BwdState& s) {   // the one-wave-per-tile dW kernel (both short-M families)
  // forked only with a workspace to book it under: the kernel itself needs none, but gt_overlap_dw_release(range) is how the
  // caller learns when the dy / mask this GEMM reads (they live in the caller's workspace) may be overwritten
  hipStream_t stream = dw_fork(c, s.dx_splits <= 1 && c.workspace && c.workspace_bytes);
  SmallArgs sa{};
  sa.x = (const float*)c.x; sa.w = c.weight; sa.dy = (const float*)c.dy; sa.ymask = (const float*)s.ymask;
  sa.M = c.M; sa.N = c.N; sa.K = c.K; sa.ldx = c.ldx; sa.ldy = c.ldy; sa.inv_keep = s.inv_keep;
  sa.out = c.dweight; sa.db = c.dbias;
  {
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_small_dw", stream, LIN_DIMS(c));
    small_launch(SMALL_DW, c.compute, gt_cdiv(c.N, 32) * gt_cdiv(c.K, 16), c.M, stream, sa);
  }
  dw_book(c, stream);
}
// "High" only: the weight gradient of a SHORT-M call on a bound weight.  k_small_dw has no three-product form (it multiplies in fp32), the
// pipelined split kernel has, and it takes any M (its M range is cut into 32-row stages): from one whole stage on (M >= 32) the dW of a
// call that would otherwise run k_small_dw runs k_lin3r_dw<.., HI> -- one split per 256 rows, within what the caller's workspace (sized as
// for compute = 0) holds.  Below 32 rows, without a bound image or a workspace, and under compute = 0 / 1, nothing changes: k_small_dw.
bool high_small_dw_ok(int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, int groups) {
  if (M < 32 || !small_eligible(x_dtype, y_dtype, M, N, K, ldx, ldy, groups) || !w3_lookup(weight, N, K, false)) return false;
  L32DwArgs d{};
  d.N = N; d.K = K; d.ldy = ldy; d.ldx = ldx;
  return w3r_dw_ok(y_dtype, x_dtype, d);
}
int bwd_high_small_dw(const LinBwd& c, BwdState& s) {
  const int64_t M = c.M, N = c.N, K = c.K;
  if (!c.high || !s.dw || c.x2 || c.map.rows || !c.workspace || c.workspace_bytes < s.need ||
      !high_small_dw_ok(c.x_dtype, c.y_dtype, c.weight, M, N, K, c.ldx, c.ldy, c.groups))
    return GT_OK;
  L32DwArgs d{};
  d.dy = c.dy; d.ymask = s.ymask; d.x = c.x; d.inv_keep = s.inv_keep;
  d.M = M; d.N = N; d.K = K; d.ldy = c.ldy; d.ldx = c.ldx; d.high = 1;
  if (!w3r_dw_ok(c.y_dtype, c.x_dtype, d)) return GT_OK;   // (the operands' alignment)
  hipStream_t stream = dw_fork(c, true);
  d.nkb = (int)gt_cdiv(K, W3D_T); d.nnb = (int)gt_cdiv(N, W3D_T);
  int splits = w3_dw_splits(M, d.nkb * d.nnb);
  const int cap = dw_splits(M, N, K, GT_F32);   // the workspace holds this many partial copies (gt_linear_bwd_workspace_bytes)
  if (splits > cap) splits = cap;
  d.m_per_split = gt_cdiv(gt_cdiv(M, splits), 32) * 32;
  d.part = reinterpret_cast<float*>(c.workspace);
  d.dbpart = c.dbias ? d.part + (size_t)splits * N * K : nullptr;
  d.splits = splits;
  dim3 grid((unsigned)(gt_cdiv(splits, 8) * 8 * d.nkb * d.nnb));
  {
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin3r_dw", stream, LIN_DIMS(c));
    w3r_launch_dw(grid, stream, d);
  }
  dw_reduce(stream, false, d.part, splits, N * K, c.dweight, d.dbpart, c.dbias ? N : 0, c.dbias);
  dw_book(c, stream);
  s.dw = false;
  return GT_OK;
}
int bwd_small(const LinBwd& c, BwdState& s) {   // short M (linear_small.h): no LDS, no partials
  if (!small_eligible(c.x_dtype, c.y_dtype, c.M, c.N, c.K, c.ldx, c.ldy, c.groups)) return GT_OK;
  if (s.dx) {
    hipStream_t stream = c.stream;
    SmallArgs sa{};
    sa.w = c.weight; sa.dy = (const float*)c.dy; sa.ymask = (const float*)s.ymask; sa.add1 = (const float*)c.dx_add1; sa.add2 = (const float*)c.dx_add2;
    sa.M = c.M; sa.N = c.N; sa.K = c.K; sa.ldx = c.ldx; sa.ldy = c.ldy; sa.inv_keep = s.inv_keep; sa.out = (float*)c.dx;
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_small_dx", stream, LIN_DIMS(c));
    small_launch(SMALL_DX, c.compute, gt_cdiv(c.M, 16) * gt_cdiv(c.K, 32), c.N, stream, sa);
  }
  if (s.dw) small_dw(c, s);
  s.dx = s.dw = false;
  return GT_OK;
}
// dX of a grouped big-M fp32 GEMM on the bound images of the groups' W^T (k_lin3, blockIdx.y = group)
int bwd_grouped3_dx(const LinBwd& c, BwdState& s) {
  if (!s.dx || c.groups <= 1 || !g3_eligible(c.compute, c.x_dtype, c.y_dtype, c.M, c.N, c.K, c.ldx, c.ldy) || c.bn_part || c.bcast || c.gate_out || c.dx2 ||
      c.map.rows)
    return GT_OK;
  int64_t spacing = 0;
  const void* img = w3_lookup_grouped(c.weight, c.N, c.K, c.groups, true, &spacing);
  if (!img) return GT_OK;
  hipStream_t stream = c.stream;
  L32Args w{};
  w.a = c.dy; w.amask = s.ymask; w.out = c.dx; w.add1 = c.dx_add1; w.add2 = c.dx_add2;
  w.M = c.M; w.Nout = c.K; w.Kc = c.N; w.lda = c.ldy; w.ldw = c.N; w.ldo = c.ldx; w.inv_keep = s.inv_keep;
  w.w3 = img; w.groups = c.groups; w.g_a = c.y_group_stride; w.g_o = c.x_group_stride; w.g_img = spacing;
  w.high = c.high;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin3[dx]", stream, LIN_DIMS(c));
  w3_launch<true>(c.y_dtype, c.x_dtype, stream, w);
  s.dx = false;
  return GT_OK;
}
// the groups' weight gradients on the pipelined bf16x6 kernel (k_lin3r_dw, blockIdx.y = group) when their weights are bound
int bwd_grouped3_dw(const LinBwd& c, BwdState& s) {
  const int64_t M = c.M, N = c.N, K = c.K;
  if (!s.dw || c.groups <= 1 || !g3_eligible(c.compute, c.x_dtype, c.y_dtype, M, N, K, c.ldx, c.ldy) || c.x2 || c.map.rows || !c.workspace ||
      c.workspace_bytes < s.need)
    return GT_OK;
  int64_t spacing = 0;
  L32DwArgs d{};
  d.dy = c.dy; d.ymask = s.ymask; d.x = c.x; d.inv_keep = s.inv_keep;
  d.M = M; d.N = N; d.K = K; d.ldy = c.ldy; d.ldx = c.ldx;
  d.groups = c.groups; d.g_y = c.y_group_stride; d.g_x = c.x_group_stride;
  d.high = c.high;
  if (!w3_lookup_grouped(c.weight, N, K, c.groups, false, &spacing) || !w3r_dw_ok(c.y_dtype, c.x_dtype, d)) return GT_OK;
  // (the weight gradient alone goes to the overlap stream: a dX that the generic kernels below still owe stays on the caller's)
  hipStream_t stream = dw_fork(c, true);
  const int shape = w3r_dw_pick_shape(N, K);
  const int nkb3 = (int)gt_cdiv(K, w3r_dw_xt(shape)), nnb3 = (int)gt_cdiv(N, w3r_dw_zt(shape));
  int s3 = w3_dw_splits(M, nkb3 * nnb3 * c.groups);
  const int cap = w32_dw_splits(M, (int)gt_cdiv(K, 64), (int)gt_cdiv(gt_cdiv(N, 16), w32_pick_nt(N)), false);   // a group's share of the workspace holds this many partial copies
  if (s3 > cap) s3 = cap;
  float* base = reinterpret_cast<float*>(c.workspace);
  d.g_part = s.g_part;
  d.part = base; d.dbpart = c.dbias ? base + (int64_t)s3 * N * K : nullptr;
  d.splits = s3; d.nkb = nkb3; d.nnb = nnb3;
  d.m_per_split = gt_cdiv(gt_cdiv(M, s3), 32) * 32;
  dim3 grid3((unsigned)(gt_cdiv(s3, 8) * 8 * nkb3 * nnb3), (unsigned)c.groups);
  {   // (the bracket holds the GEMM kernel alone: one rocprofv3 row; its fixed-order reduce is k_split_reduce's row)
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin3r_dw", stream, LIN_DIMS(c));
    w3r_launch_dw(grid3, stream, d, shape);
  }
  // (reduced right behind the GEMM, not deferred to the end of the backward: the PNA driver gathers the image gradients before that)
  const int64_t len = N * K, len2 = c.dbias ? N : 0;
  const int rg = (int)(gt_cdiv(len + len2, 256) < 2048 ? gt_cdiv(len + len2, 256) : 2048);
  hipLaunchKernelGGL(k_split_reduce, dim3(rg, c.groups), dim3(256), 0, stream, (const float*)base, s3, len, c.dweight, (const float*)d.dbpart,
                     len2, c.dbias, d.g_part);
  dw_book(c, stream);
  s.dw = false;
  return GT_OK;
}
// dX = dZ (W^T)^T of the big-M exact-fp32 path: the forward-form kernel on the transposed weight; wt = where the workspace holds W^T
int wide_dx(const LinBwd& c, const BwdState& s, float* wt) {
  const int64_t M = c.M, N = c.N, K = c.K;
  hipStream_t stream = c.stream;
  const auto fail = [](const char* msg) { gt_set_error("%s", msg); return GT_ERR_UNSUPPORTED; };
  const void* w3t = (c.y_dtype != GT_F32 && N % 8) ? nullptr : w3_lookup(c.weight, N, K, true);
  if (c.bn_part) {   // which kernel's epilogue sums the statistics: the one that writes as many partial rows as the buffer was sized for
    // (lin_bwd has checked the count: 0, or one of the two kernels'; where the two coincide it names neither and the option decides)
    const int64_t rows_kernel = gt_cdiv(M, 128), exact = gt_cdiv(M, W32_BM);
    bool on_rows = c.bn_nparts == rows_kernel;
    if (c.bn_nparts == 0 || rows_kernel == exact) on_rows = bns_on_rows_kernel(c.x_dtype, c.y_dtype, c.weight, M, N, K, c.ldx, c.ldy);
    else if (on_rows && (!w3t || !bns_rows_kernel_can(c.x_dtype, c.y_dtype, c.weight, M, N, K, c.ldx, c.ldy)))
      return fail("gt_linear_bwd: BatchNorm partials sized for the register-row kernel, which does not take this call");
    if (!on_rows) w3t = nullptr;   // the exact kernel's epilogue then
  }
  if (w3t) {
    wt = nullptr;   // the bound image of W^T: k_lin3, no transpose
  } else if (c.weight_t) {
    wt = const_cast<float*>(c.weight_t);   // read only
  } else {
    // W^T lives in the caller's workspace: a previous call's dW GEMM may still be running on the overlap stream with
    // its partials in the same workspace (callers hand ONE workspace to consecutive GEMMs, e.g. the four of an encoder
    // layer) -> wait for the forks that used this range (those on other workspaces keep running).
    if (g_dw.active && stream == g_dw.main) dw_release(c.workspace, c.workspace_bytes);
    hipLaunchKernelGGL(k_transpose32, dim3((unsigned)gt_cdiv(K, 32), (unsigned)gt_cdiv(N, 32)), dim3(256), 0, stream, c.weight, wt, N, K);
  }
  L32Args w{};
  w.a = c.dy; w.amask = s.ymask; w.w = wt; w.out = c.dx; w.add1 = c.dx_add1; w.add2 = c.dx_add2;
  w.M = M; w.Nout = K; w.Kc = N; w.lda = c.ldy; w.ldw = N; w.ldo = c.ldx; w.inv_keep = s.inv_keep;
  w.high = c.high;
  if (c.bn_part && c.x_dtype == GT_F32 && c.y_dtype == GT_F32) {
    w.bn_x = c.bn_x; w.bn_ldx = c.bn_ldx; w.bn_mean = c.bn_mean; w.bn_rstd = c.bn_rstd; w.bn_w = c.bn_w; w.bn_b = c.bn_b;
    w.bn_relu = c.bn_relu; w.bn_part = c.bn_part;
  }
  w.w3 = w3t;
  if (c.bcast) {
    w.add_bc = c.bcast; w.add_bidx = c.bcast_idx;
    if (!w3t || !w3r_ok(c.y_dtype, c.x_dtype, w)) return fail("gt_linear_bwd_bcast: this call does not run on the register-row kernel (ask gt_linear_bwd_bcast_ok)");
  }
  if (c.map.rows) {
    if (!w3t) return fail("gt_linear_set_rows: needs the bound image of W^T");
    w.a_rows = c.map.rows;
  }
  if (c.dx2) {
    if (!w3t || c.dx_add1 || c.dx_add2) return fail("gt_linear_bwd_cat2: needs a bound weight image and no addends");
    w.out2 = c.dx2; w.out_split = c.x_split; w.ldo2 = c.ldx2;
  }
  const bool on_rows_kernel = w3t && w3r_ok(c.y_dtype, c.x_dtype, w);
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, on_rows_kernel ? "k_lin3r[dx]" : (w3t ? "k_lin3[dx]" : "k_lin32[dx]"), stream, LIN_DIMS(c));
  if (on_rows_kernel) w3r_launch(stream, w);
  else if (w3t) w3_launch<true>(c.y_dtype, c.x_dtype, stream, w);
  else w32_launch<true>(c.y_dtype, c.x_dtype, stream, w);
  return GT_OK;
}
// dW of the big-M exact-fp32 path, split over M: the bf16x6 kernels on a bound weight (k_lin3r_dw / k_lin3_dw), else k_lin32_dw
int wide_dw(const LinBwd& c, const BwdState& s, hipStream_t stream, float* part, int splits, int nt, int nkb, int nnb) {
  const int64_t M = c.M, N = c.N, K = c.K;
  L32DwArgs d{};
  d.dy = c.dy; d.ymask = s.ymask; d.x = c.x; d.inv_keep = s.inv_keep;
  d.M = M; d.N = N; d.K = K; d.ldy = c.ldy; d.ldx = c.ldx;
  if (c.x2) { d.x2 = c.x2; d.x_split = c.x_split; d.ldx2 = c.ldx2; }
  d.high = c.high;
  // weights with bound images run the bf16x6 dW kernel too (160 x 160 output tiles, split over M; linear3x.h)
  const bool split3 = c.x_dtype == GT_F32 && w3_lookup(c.weight, N, K, false) != nullptr && (c.y_dtype == GT_F32 || N % 8 == 0);
  if (c.map.rows && !split3) { gt_set_error("gt_linear_set_rows: needs the bound weight image"); return GT_ERR_UNSUPPORTED; }
  d.dy_rows = c.map.rows;
  if (split3) {
    d.nkb = (int)gt_cdiv(K, W3D_T); d.nnb = (int)gt_cdiv(N, W3D_T);
    splits = w3_dw_splits(M, d.nkb * d.nnb);
    const int cap = w32_dw_splits(M, nkb, nnb, false);   // the workspace is sized for this many partial copies
    if (splits > cap) splits = cap;
    d.m_per_split = gt_cdiv(gt_cdiv(M, splits), 32) * 32;
  } else {
    d.nkb = nkb; d.nnb = nnb;
    d.m_per_split = gt_cdiv(gt_cdiv(M, splits), 16) * 16;
  }
  bool deferred;
  d.part = dw_part(part, splits, N, K, &deferred);
  d.dbpart = c.dbias ? d.part + (size_t)splits * N * K : nullptr;
  d.splits = splits;
  dim3 grid((unsigned)(gt_cdiv(splits, 8) * 8 * d.nkb * d.nnb));
  const bool pipelined = split3 && w3r_dw_ok(c.y_dtype, c.x_dtype, d);
  {
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, pipelined ? "k_lin3r_dw" : (split3 ? "k_lin3_dw" : "k_lin32_dw"), stream, LIN_DIMS(c));
    if (pipelined) w3r_launch_dw(grid, stream, d);   // stages pipelined (linear3r.h)
    else if (split3 && c.y_dtype == GT_F32) w3_launch_dw<float, float>(grid, stream, d);
    else if (split3) w3_launch_dw<gt_bf16, float>(grid, stream, d);
    else if (c.y_dtype == GT_F32) w32_launch_dw_nt<float, float>(nt, grid, stream, d);
    else w32_launch_dw_nt<gt_bf16, float>(nt, grid, stream, d);
  }
  dw_reduce(stream, deferred, d.part, splits, N * K, c.dweight, d.dbpart, c.dbias ? N : 0, c.dbias);
  return GT_OK;
}
int bwd_wide(const LinBwd& c, BwdState& s) {   // big-M exact-fp32 compute (linear32.h, linear3x.h, linear3r.h): dX and dW
  if (!w32_eligible(c.compute, c.x_dtype, c.M, c.groups)) return GT_OK;
  const int64_t M = c.M, N = c.N, K = c.K;
  if (!c.workspace || c.workspace_bytes < s.need) {
    gt_set_error("gt_linear_bwd: workspace too small (%zu < %zu)", c.workspace_bytes, s.need);
    return GT_ERR_WORKSPACE;
  }
  const int nt = w32_pick_nt(N);
  const int nkb = (int)gt_cdiv(K, 64), nnb = (int)gt_cdiv(gt_cdiv(N, 16), nt);
  // (a weight gradient that will share the chip with the critical path runs fewer splits, unless the optimizer waits for it: w32_dw_splits)
  const int splits = w32_dw_splits(M, nkb, nnb, dw_will_fork(c, s.dw) && !g_dw.urgent);
  float* part = reinterpret_cast<float*>(c.workspace);
  float* wt = part + (size_t)w32_dw_splits(M, nkb, nnb, false) * (size_t)(N * K + N) + 64;   // behind the larger partial area
  wt = reinterpret_cast<float*>(((uintptr_t)wt + 255) & ~(uintptr_t)255);
  if (s.dx)
    if (const int rc = wide_dx(c, s, wt)) return rc;
  if (s.dw) {
    hipStream_t stream = dw_fork(c, true);
    if (const int rc = wide_dw(c, s, stream, part, splits, nt, nkb, nnb)) return rc;
    dw_book(c, stream);
  }
  s.dx = s.dw = false;
  return GT_OK;
}
// dX = dY W on the bound image of W^T (linear1.h / linear2.h); a gate here applies to the OUTPUT columns (gt_linear_bwd_gate_out)
int bwd_bf16_image_dx(const LinBwd& c, BwdState& s) {
  if (!s.dx || c.x_dtype != GT_BF16 || c.y_dtype != GT_BF16 || c.compute != GT_BF16 || c.groups != 1 || c.M < W1_MIN_M || (c.y_for_mask && !c.gate_out))
    return GT_OK;
  const void* img = w1_lookup(c.weight, c.N, c.K, true);
  if (!img) return GT_OK;
  hipStream_t stream = c.stream;
  L1Args l{};
  l.a = (const gt_bf16*)c.dy; l.img = (const unsigned char*)img; l.out = (gt_bf16*)c.dx;
  l.gate = c.gate_out ? (const gt_bf16*)c.y_for_mask : nullptr; l.gate_inv_keep = s.inv_keep;
  l.add1 = (const gt_bf16*)c.dx_add1; l.add2 = (const gt_bf16*)c.dx_add2;
  l.M = c.M; l.lda = c.ldy; l.ldo = c.ldx; l.N = (int)c.K; l.K = (int)c.N;
  const bool ring = w2_take(l, w1_pick_ntw(c.K, c.N) != 0);
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, ring ? "k_lin2[dx]" : "k_lin1[dx]", stream, LIN_DIMS(c));
  s.dx = !(ring ? w2_launch(stream, l) : w1_launch(stream, l));
  return GT_OK;
}
// gt_linear_bwd_gate_out: only the family above gates the dX output; behind it the gate is spent
int bwd_gate_out_spent(const LinBwd& c, BwdState& s) {
  if (!c.gate_out) return GT_OK;
  if (s.dx) { gt_set_error("gt_linear_bwd_gate_out: not covered (ask gt_linear_bwd_gate_out_ok)"); return GT_ERR_UNSUPPORTED; }
  s.ymask = nullptr;   // the gate belongs to the dX output, not to dY: the weight gradient below reads dY as it is
  return GT_OK;
}
// the prediction heads: the contraction is their 25 010 columns (linear_heads.h)
// (shape matching alone must not route a general GEMM with per-call options here: k_heads_dx knows none of them)
int bwd_heads_dx(const LinBwd& c, BwdState& s) {
  if (!s.dx || s.ymask || c.mul_mask || c.bn_part || c.gate_out || c.dropout_p != 0.f ||
      !heads_shape_ok(c.x_dtype, c.y_dtype, c.M, c.N, c.K, c.ldx, c.ldy, c.groups) || !c.workspace ||
      c.workspace_bytes < heads_dx_workspace_bytes(c.M, c.N))
    return GT_OK;
  hipStream_t stream = c.stream;
  HeadsArgs h{};
  h.w = c.weight; h.dy = (const float*)c.dy; h.M = c.M; h.N = c.N; h.ldx = c.ldx; h.ldy = c.ldy;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_heads_dx+reduce", stream, LIN_DIMS(c));
  heads_launch_dx(c.compute, stream, h, c.workspace, (float*)c.dx, (const float*)c.dx_add1, (const float*)c.dx_add2);
  s.dx = false;
  return GT_OK;
}
LinArgs tiled_args(const LinBwd& c, const BwdState& s) {
  LinArgs a{};
  a.w = c.weight; a.a = c.dy; a.ymask = s.ymask; a.x = c.x; a.M = c.M; a.N = c.N; a.K = c.K; a.ldy = c.ldy; a.ldx = c.ldx;
  a.add1 = c.dx_add1; a.add2 = c.dx_add2; a.inv_keep = s.inv_keep;
  a.g_x = c.x_group_stride; a.g_y = c.y_group_stride; a.g_w = c.N * c.K; a.g_b = c.N; a.g_part = s.g_part;
  return a;
}
int bwd_tiled_dx(const LinBwd& c, BwdState& s) {
  if (!s.dx) return GT_OK;
  const int64_t M = c.M, N = c.N, K = c.K;
  hipStream_t stream = c.stream;
  const int compute = c.compute, bm = pick_bm(M);
  // split-N partials are plain fp32 sums: only for fp32 dX without fused addends (and not for grouped launches)
  int splits = (c.x_dtype == GT_F32 && !c.dx_add1 && !c.dx_add2 && c.ldx == K && c.groups == 1) ? dx_splits(M, N, K, bm) : 1;
  if (splits > 1 && (!c.workspace || c.workspace_bytes < s.need)) splits = 1;
  LinArgs a = tiled_args(c, s);
  a.splits = splits;
  a.n_per_split = gt_cdiv(gt_cdiv(N, splits), 64) * 64;
  a.out = splits > 1 ? c.workspace : c.dx;
  a.ntiles = (int)gt_cdiv(K, BN);
  dim3 grid((unsigned)(gt_cdiv(gt_cdiv(M, bm), 8) * 8 * a.ntiles), (unsigned)c.groups, (unsigned)splits);
  const int t0 = c.y_dtype, t1 = c.x_dtype;
  GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_linear_dx", stream, LIN_DIMS(c));
  if (bm == 64) GT_LIN_DISPATCH_BM(k_linear_dx, 64, grid, a);
  else GT_LIN_DISPATCH_BM(k_linear_dx, 128, grid, a);
  if (splits > 1) {
    const int64_t len = M * K;
    const int rg = (int)(gt_cdiv(len, 256) < 2048 ? gt_cdiv(len, 256) : 2048);
    hipLaunchKernelGGL(k_split_reduce, dim3(rg), dim3(256), 0, stream, (const float*)c.workspace, splits, len,
                       reinterpret_cast<float*>(c.dx), (const float*)nullptr, (int64_t)0, (float*)nullptr, (int64_t)0);
  }
  s.dx = false;
  s.dx_splits = splits;
  return GT_OK;
}
int bwd_small_wide_dw(const LinBwd& c, BwdState& s) {   // wide short-M GEMM: dW on the one-wave-per-tile kernel
  if (!s.dw || !small_wide_ok(c.x_dtype, c.y_dtype, c.M, c.K, c.ldx, c.ldy, c.groups)) return GT_OK;
  small_dw(c, s);
  s.dw = false;
  return GT_OK;
}
// dW split over M with a fixed-order reduce: bf16 token rows on the LDS-DMA ring kernel (linear_dw16.h), everything else on the tiled one
int bwd_split_dw(const LinBwd& c, BwdState& s) {
  if (!s.dw) return GT_OK;
  const int64_t M = c.M, N = c.N, K = c.K;
  const int compute = c.compute, splits = dw_splits(M, N, K, compute);
  if (!c.workspace || c.workspace_bytes < s.need) {
    gt_set_error("gt_linear_bwd: workspace too small (%zu < %zu)", c.workspace_bytes, s.need);
    return GT_ERR_WORKSPACE;
  }
  hipStream_t stream = dw_fork(c, s.dx_splits <= 1);
  if (dw16_ok(c.x_dtype, c.y_dtype, compute, c.x, c.dy, s.ymask, M, N, K, c.ldx, c.ldy, c.groups)) {
    Dw16Args d{};
    d.dy = (const gt_bf16*)c.dy; d.x = (const gt_bf16*)c.x; d.M = M; d.N = N; d.K = K; d.ldy = c.ldy; d.ldx = c.ldx;
    d.splits = dw16_splits(M, N, K, splits);
    d.m_per_split = gt_cdiv(gt_cdiv(M, d.splits), D16_ROWS) * D16_ROWS;
    bool deferred;
    d.part = dw_part(reinterpret_cast<float*>(c.workspace), d.splits, N, K, &deferred);
    d.dbpart = c.dbias ? d.part + (size_t)d.splits * N * K : nullptr;
    d.ntx = (int)(N / D16_T);
    d.ntiles = d.ntx * (int)(K / D16_T);
    {
      GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_dw16", stream, LIN_DIMS(c));
      hipLaunchKernelGGL(k_dw16, dim3((unsigned)(gt_cdiv(d.splits, 8) * 8 * d.ntiles)), dim3(256), 0, stream, d);
    }
    dw_reduce(stream, deferred, d.part, d.splits, N * K, c.dweight, d.dbpart, c.dbias ? N : 0, c.dbias);
  } else {
    const int64_t bmc = compute == GT_BF16 ? 64 : 32;
    LinArgs a = tiled_args(c, s);
    a.splits = splits;
    a.m_per_split = gt_cdiv(gt_cdiv(M, splits), bmc) * bmc;
    a.out = c.workspace;
    a.dbpart = c.dbias ? reinterpret_cast<float*>(c.workspace) + (size_t)splits * N * K : nullptr;
    a.ntx = (int)gt_cdiv(N, BN);
    a.ntiles = a.ntx * (int)gt_cdiv(K, BN);
    dim3 grid((unsigned)(gt_cdiv(splits, 8) * 8 * a.ntiles), (unsigned)c.groups);
    const int t0 = c.y_dtype, t1 = c.x_dtype;
    {
      GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_linear_dw", stream, LIN_DIMS(c));
      GT_LIN_DISPATCH(k_linear_dw, grid, a);
    }
    const int64_t len = N * K, len2 = c.dbias ? N : 0;
    const int rg = (int)(gt_cdiv(len + len2, 256) < 2048 ? gt_cdiv(len + len2, 256) : 2048);
    hipLaunchKernelGGL(k_split_reduce, dim3(rg, c.groups), dim3(256), 0, stream, (const float*)c.workspace, splits, len, c.dweight,
                       (const float*)a.dbpart, len2, c.dbias, a.g_part);
  }
  dw_book(c, stream);
  s.dw = false;
  return GT_OK;
}
}  // namespace

int lin_bwd(const LinBwd& c_) {
  const char* fn = "gt_linear_bwd_grouped";
  LinBwd c = c_;   // (the one place a backward's `compute` is normalised: linear_call.h)
  c.high = c.compute == GT_COMPUTE_F32_HIGH;
  c.compute = gt_compute_base(c.compute);
  if (c.bcast && c.dx && !gt_linear_bwd_bcast_ok(c.compute, c.x_dtype, c.y_dtype, c.weight, c.M, c.N, c.K)) {
    gt_set_error("gt_linear_bwd_bcast: this call does not run on the register-row kernel (ask gt_linear_bwd_bcast_ok)");
    return GT_ERR_UNSUPPORTED;
  }
  LIN_CHECK_ARG(fn, !c.map.add_table, "gt_linear_set_rows_add: forward only (a constant addend has no backward)");
  LIN_CHECK_ARG(fn, !c.bn_part || c.bn_nparts == 0 || c.bn_nparts == gt_cdiv(c.M, 128) || c.bn_nparts == gt_cdiv(c.M, W32_BM),
                "BatchNorm partial rows (bn_nparts) fit neither dX kernel: ceil(M / 128) or ceil(M / 64)");
  LIN_CHECK_ARG(fn, !c.map.rows || (c.groups == 1 && !c.y_for_mask && !c.bn_part && !c.map.ln_out &&
                                    rows_eligible(c.compute, c.x_dtype, c.y_dtype, c.weight, c.M, c.N, c.K)),
                "gt_linear_set_rows: this GEMM does not take a row map (ask gt_linear_rows_ok)");
  int rc = check_call(fn, "gt_linear_bwd", c.x_dtype, c.y_dtype, c.compute, c.M, c.N, c.K, c.ldx, c.ldy, c.x2 ? c.x_split : c.K, c.groups,
                      c.x_group_stride, c.y_group_stride);
  if (rc) return rc;
  LIN_CHECK_ARG(fn, c.weight && c.dy, "null buffer");
  LIN_CHECK_ARG(fn, c.dx || c.dweight, "nothing to compute");
  LIN_CHECK_ARG(fn, !c.dweight || c.x, "dweight needs x");
  LIN_CHECK_ARG(fn, c.dropout_p >= 0.f && c.dropout_p < 1.f, "dropout_p must be in [0,1)");
  GtProfScope prof__(GT_PROF_LINEAR, c.dx ? (c.dweight ? "gt_linear_bwd" : "gt_linear_bwd_dx") : "gt_linear_bwd_dw", c.stream, LIN_DIMS(c));
  if (c.M == 0) {
    if (c.dweight) (void)hipMemsetAsync(c.dweight, 0, (size_t)c.groups * c.N * c.K * sizeof(float), c.stream);
    if (c.dbias) (void)hipMemsetAsync(c.dbias, 0, (size_t)c.groups * c.N * sizeof(float), c.stream);
    return GT_OK;
  }
  const size_t need1 = gt_linear_bwd_workspace_bytes(c.compute, c.M, c.N, c.K);   // per group
  BwdState s{};
  s.dx = c.dx != nullptr; s.dw = c.dweight != nullptr; s.ymask = c.y_for_mask;
  s.inv_keep = c.mul_mask ? 0.f : 1.0f / (1.0f - c.dropout_p);
  s.need = (size_t)c.groups * need1;
  s.g_part = (int64_t)(need1 / sizeof(float));
  static int (*const families[])(const LinBwd&, BwdState&) = {
      bwd_high_small_dw, bwd_small, bwd_grouped3_dx, bwd_grouped3_dw, bwd_wide, bwd_bf16_image_dx, bwd_gate_out_spent, bwd_heads_dx, bwd_tiled_dx, bwd_small_wide_dw,
      bwd_split_dw};
  for (auto family : families) {
    if ((rc = family(c, s)) != GT_OK) return rc;
    if (!s.dx && !s.dw) break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { gt_set_error("%s: launch failed: %s", fn, hipGetErrorString(e)); return GT_ERR_LAUNCH; }
  return GT_OK;
}

extern "C" int gt_linear_bwd(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy, const void* y_for_mask,
                             const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K,
                             float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  return gt_linear_bwd_grouped(x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, K, N, 1, 0, 0,
                               dropout_p, workspace, workspace_bytes, stream_);
}

extern "C" int gt_linear_bwd_ld(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy, const void* y_for_mask,
                                const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K,
                                int64_t ldy, float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  return gt_linear_bwd_grouped(x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, K, ldy, 1, 0, 0,
                               dropout_p, workspace, workspace_bytes, stream_);
}

extern "C" int gt_linear_bwd_ld2(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy, const void* y_for_mask,
                                 const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K,
                                 int64_t ldx, int64_t ldy, float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  return gt_linear_bwd_grouped(x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, dx_add1, dx_add2, dx, dweight, dbias, M, N, K,
                               ldx, ldy, 1, 0, 0, dropout_p, workspace, workspace_bytes, stream_);
}

extern "C" int gt_linear_bwd_grouped(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy,
                                     const void* y_for_mask, const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias,
                                     int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, int groups, int64_t x_group_stride,
                                     int64_t y_group_stride, float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, ldx, ldy, groups,
               x_group_stride, y_group_stride, dropout_p, workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  return lin_bwd(c);
}

// W^T [K][N] supplied by the caller (one gt_transpose per weight and backward pass instead of one in front of every wide fp32 dX GEMM)
extern "C" int gt_linear_bwd_wt(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const float* weight_t, const void* dy,
                                const void* y_for_mask, const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias, int64_t M,
                                int64_t N, int64_t K, float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, K, N, 1, 0, 0, dropout_p,
               workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.weight_t = weight_t;
  return lin_bwd(c);
}

// dW / db only, inside a gt_overlap_dw section still on the overlap stream: a caller can start a GEMM's weight gradient BEFORE its dX GEMM
// (the encoder layer's in_proj: a dW GEMM that starts together with the next layer's first kernel is what the fused backward avoids)
extern "C" int gt_linear_bwd_dw_forked(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy,
                                       const void* y_for_mask, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K, int64_t ldx,
                                       int64_t ldy, float dropout_p, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, y_for_mask, nullptr, nullptr, nullptr, dweight, dbias, M, N, K, ldx, ldy, 1, 0, 0,
               dropout_p, workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.fork_dw_only = true;
  return lin_bwd(c);
}

// gt_linear_bwd_dw_forked for a layer whose forward saved a multiplier (gt_linear_fwd_gelu): dZ = dY * gmul
extern "C" int gt_linear_bwd_mul_dw_forked(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy,
                                           const void* gmul, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy,
                                           void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  GT_CHECK_ARG(gmul, "gt_linear_bwd_mul_dw_forked needs the multiplier");
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, gmul, nullptr, nullptr, nullptr, dweight, dbias, M, N, K, ldx, ldy, 1, 0, 0, 0.f,
               workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.fork_dw_only = true;
  c.mul_mask = true;
  return lin_bwd(c);
}

// backward of gt_linear_fwd_gelu: `gmul` is the multiplier that forward saved (dZ = dY * gmul); everything else as gt_linear_bwd_ld2
extern "C" int gt_linear_bwd_mul(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy, const void* gmul,
                                 const void* dx_add1, const void* dx_add2, void* dx, float* dweight, float* dbias, int64_t M, int64_t N, int64_t K,
                                 int64_t ldx, int64_t ldy, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  GT_CHECK_ARG(gmul, "gt_linear_bwd_mul needs the multiplier");
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, gmul, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, ldx, ldy, 1, 0, 0, 0.f, workspace,
               workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.mul_mask = true;
  return lin_bwd(c);
}

// ---- JK = "cat" without the copy: X = [X1 | X2] (modules/gnn_module.py:104-105 feeding models/gnn_transformer.py:92) -------------
// 1 when gt_linear_fwd_cat2 / gt_linear_bwd_cat2 can run this GEMM (big-M exact-fp32 compute on a weight whose images are bound)
extern "C" int gt_linear_cat2_ok(int compute, const float* weight, int64_t M, int64_t N, int64_t K1, int64_t K2) {
  return (w32_eligible(compute, GT_F32, M, 1) && K1 > 0 && K2 > 0 && K1 % 4 == 0 && K2 % 4 == 0 && w3_lookup(weight, N, K1 + K2, false) &&
          w3_lookup(weight, N, K1 + K2, true)) ? 1 : 0;
}
// ---- a row map on the output (forward) / on dY (backward): gnn2transformer writing and reading the Transformer's token rows in place
// (models/gnn_transformer.py:92-96, modules/utils.py:5-29: no pad / unpad pass over the node rows) -----------------------------------
// bf16 products per fp32 product of a plain call under the current bindings (include/graphtrans_hip.h): the dispatchers' own tests
extern "C" int gt_linear_products(int which, int x_dtype, int y_dtype, int compute, const float* weight, int64_t M, int64_t N, int64_t K) {
  const bool high = compute == GT_COMPUTE_F32_HIGH;
  if (which < 0 || which > 2 || !weight || N <= 0 || K <= 0) return 0;
  if (which == 2 && high && gt_compute_base(compute) == GT_F32 && high_small_dw_ok(x_dtype, y_dtype, weight, M, N, K, K, N, 1)) return 3;   // bwd_high_small_dw
  if (!w32_eligible(compute, x_dtype, M, 1)) return 0;
  if (which == 0) {   // fwd_heads comes first, then fwd_wide
    if (heads_shape_ok(x_dtype, y_dtype, M, N, K, K, N, 1)) return 0;
    L32Args w{};
    w.w3 = (x_dtype == GT_F32 || K % 8 == 0) ? w3_lookup(weight, N, K, false) : nullptr;
    if (!w.w3) return 0;
    w.M = M; w.Nout = N; w.Kc = K; w.lda = K; w.ldo = N; w.high = high;
    return (w3r_ok(x_dtype, y_dtype, w) ? high : w3_high(x_dtype, y_dtype, w)) ? 3 : 6;
  }
  if (which == 1) {   // wide_dx
    L32Args w{};
    w.w3 = (y_dtype != GT_F32 && N % 8) ? nullptr : w3_lookup(weight, N, K, true);
    if (!w.w3) return 0;
    w.M = M; w.Nout = K; w.Kc = N; w.lda = N; w.ldo = K; w.high = high;
    return (w3r_ok(y_dtype, x_dtype, w) ? high : w3_high(y_dtype, x_dtype, w)) ? 3 : 6;
  }
  // wide_dw
  if (!(x_dtype == GT_F32 && w3_lookup(weight, N, K, false) != nullptr && (y_dtype == GT_F32 || N % 8 == 0))) return 0;
  L32DwArgs d{};
  d.M = M; d.N = N; d.K = K; d.ldy = N; d.ldx = K; d.high = high;
  return (w3r_dw_ok(y_dtype, x_dtype, d) && w3r_dw_high(d)) ? 3 : 6;
}

extern "C" int gt_linear_rows_ok(int compute, int x_dtype, int y_dtype, const float* weight, int64_t M, int64_t N, int64_t K) {
  return (rows_eligible(compute, x_dtype, y_dtype, weight, M, N, K)) ? 1 : 0;
}
extern "C" int gt_linear_set_rows(const int32_t* rows) {
  g_pending.map.rows = rows;
  return GT_OK;
}
// ... and LayerNorm(ln_w, ln_b, eps) of every stored row in the same epilogue (forward only): ln_out (storage type and pitch of y) gets
// the normalised row, ln_mean / ln_rstd its statistics, all at the row the output goes to.  N must fill one column block of the kernel.
extern "C" int gt_linear_rows_layernorm_ok(int64_t N) { return (N > 0 && N % 16 == 0 && (int64_t)w3_pick_nt(N) * 16 == N) ? 1 : 0; }
extern "C" int gt_linear_set_rows_layernorm(const int32_t* rows, const float* ln_w, const float* ln_b, float eps, void* ln_out, float* ln_mean,
                                            float* ln_rstd) {
  GT_CHECK_ARG(rows && ln_w && ln_b && ln_out && ln_mean && ln_rstd, "null buffer");
  LinRowMap& p = g_pending.map;   // (a pending gt_linear_set_rows_add stays)
  p.rows = rows; p.ln_w = ln_w; p.ln_b = ln_b; p.ln_out = ln_out; p.ln_mean = ln_mean; p.ln_rstd = ln_rstd; p.ln_eps = eps;
  return GT_OK;
}
// ... and a row-gathered fp32 addend for the next forward GEMM with a row map (gt_linear_set_rows / _layernorm, in either order): the
// stored row of GEMM row m is T(row m + table[idx[m]][0..N)), the sum in fp32 behind bias / activation and before the LayerNorm;
// idx[m] < 0 adds nothing.  table: fp32, 16-byte aligned, pitch ld >= N, ld % 4 == 0; idx: int32 [M] (gt_seq_positions).  Taken and
// cleared by the next public forward or backward call like the row map; a call without a row map, and every backward, refuses it.
extern "C" int gt_linear_set_rows_add(const float* table, const int32_t* idx, int64_t ld) {
  GT_CHECK_ARG(table && idx && ld > 0, "null buffer");
  g_pending.map.add_table = table; g_pending.map.add_idx = idx; g_pending.map.add_ld = ld;
  return GT_OK;
}
// Y[M][N] = [X1 | X2] W^T + b with X1 [M][K1] (pitch ldx1), X2 [M][K2] (pitch ldx2), W [N][K1 + K2]; fp32 rows, y_dtype fp32 / bf16
extern "C" int gt_linear_fwd_cat2(int y_dtype, int compute, const void* x1, int64_t K1, int64_t ldx1, const void* x2, int64_t K2, int64_t ldx2,
                                  const float* weight, const float* bias, void* y, int64_t M, int64_t N, int64_t ldy, gt_stream_t stream_) {
  LinFwd f{GT_F32, y_dtype, compute, x1, weight, bias, y, M, N, K1 + K2, ldx1, ldy, 1, 0, 0, 0, 0.f, 0, (hipStream_t)stream_};
  f.map = take_map();   // (dropped even when the check below refuses the call)
  GT_CHECK_ARG(x1 && x2 && K1 > 0 && K2 > 0 && K1 % 4 == 0 && K2 % 4 == 0 && ldx2 >= K2 && ldx2 % 4 == 0, "bad second operand");
  f.x2 = x2; f.x_split = K1; f.ldx2 = ldx2;
  return lin_fwd(f);
}
// backward of the above: dX1 [M][K1] (pitch lddx1) and dX2 [M][K2] (pitch lddx2) from dY [M][N] (y_dtype, pitch ldy); dW [N][K1+K2], db
extern "C" int gt_linear_bwd_cat2(int y_dtype, int compute, const void* x1, int64_t K1, int64_t ldx1, const void* x2, int64_t K2, int64_t ldx2,
                                  const float* weight, const void* dy, void* dx1, int64_t lddx1, void* dx2, int64_t lddx2, float* dweight,
                                  float* dbias, int64_t M, int64_t N, int64_t ldy, void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  const LinRowMap map = take_map();   // (dropped even when the checks below refuse the call)
  GT_CHECK_ARG(x1 && x2 && dx1 && dx2 && K1 > 0 && K2 > 0 && K1 % 4 == 0 && K2 % 4 == 0, "bad operands");
  GT_CHECK_ARG(ldx1 == lddx1 && ldx2 == lddx2, "dX pitches must equal the X pitches");   // (one pitch per matrix in the kernel arguments)
  LinBwd c{GT_F32, y_dtype, compute, x1, weight, dy, nullptr, nullptr, nullptr, dx1, dweight, dbias, M, N, K1 + K2, ldx1, ldy, 1, 0, 0, 0.f,
           workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.map = map;
  c.x2 = x2; c.dx2 = dx2; c.x_split = K1; c.ldx2 = ldx2;
  return lin_bwd(c);
}

// ---- bf16x3 weight images (linear3x.h) --------------------------------------------------------------------------------
// bytes of the image of a weight used as [rows][contraction] (forward: rows = N, contraction = K; dX form: rows = K, contraction = N)
extern "C" size_t gt_w3_image_bytes(int64_t rows, int64_t contraction) {
  return rows > 0 && contraction > 0 ? w3_image_bytes(rows, contraction) : 0;
}
// Builds `n` images in as few launches as the kernel-argument table allows (64 jobs each).  Job i: weight[i] is the fp32 matrix
// [N[i]][K[i]] (row pitch K[i]); transposed[i] == 0 -> image of W (rows N, contraction K) for the forward, != 0 -> image of W^T (rows K,
// contraction N) for the dX GEMM; image[i] has gt_w3_image_bytes(rows, contraction) bytes, 1024-byte aligned.
extern "C" int gt_w3_images(int n, const float* const* weight, const int64_t* N, const int64_t* K, const int* transposed,
                            void* const* image, gt_stream_t stream_) {
  GT_CHECK_ARG(n >= 0 && (n == 0 || (weight && N && K && transposed && image)), "bad arguments");
  for (int i0 = 0; i0 < n; i0 += W3_MAX_JOBS) {
    W3Jobs jobs{};
    int blocks = 0;
    const int cnt = n - i0 < W3_MAX_JOBS ? n - i0 : W3_MAX_JOBS;
    for (int i = 0; i < cnt; ++i) {
      const int s = i0 + i;
      GT_CHECK_ARG(weight[s] && image[s] && N[s] > 0 && K[s] > 0 && ((uintptr_t)image[s] & 1023) == 0, "null / unaligned buffer");
      W3Job& J = jobs.j[i];
      const int64_t rows = transposed[s] ? K[s] : N[s], contr = transposed[s] ? N[s] : K[s];
      J.w = weight[s]; J.img = (unsigned char*)image[s]; J.R = (int)rows; J.C = (int)contr; J.ldw = (int)K[s];
      J.transposed = transposed[s] ? 1 : 0; J.ntp = (int)w3_ntp(rows); J.ksteps = (int)gt_cdiv(contr, 32); J.block0 = blocks;
      blocks += J.ksteps * ((J.ntp + 3) / 4);
    }
    jobs.n = cnt;
    hipLaunchKernelGGL(k_w3_image, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, jobs);
  }
  GT_CHECK_LAUNCH();
  return GT_OK;
}
// Binds prepared images to weight pointers for the calling HOST THREAD: until gt_w3_unbind(), every big-M exact-fp32 GEMM
// (compute == GT_F32, M >= 1024, one group) of gt_linear_fwd* / gt_linear_bwd* whose weight (pointer, N, K) is in the table runs
// the bf16x6 kernel on the image (forward: image_fwd[i], dX: image_t[i]; a NULL entry keeps the exact-fp32 MFMA kernel for that
// direction).  The images must stay valid and current (rebuilt after every optimizer step) while bound.  At most 64 entries.
extern "C" int gt_w3_bind(int n, const float* const* weight, const int64_t* N, const int64_t* K, const void* const* image_fwd,
                          const void* const* image_t) {
  GT_CHECK_ARG(n >= 0 && n <= W3_MAX_BOUND && (n == 0 || (weight && N && K)), "at most 64 bound weights");
  for (int i = 0; i < n; ++i)
    g_w3.e[i] = W3Bound{weight[i], N[i], K[i], image_fwd ? image_fwd[i] : nullptr, image_t ? image_t[i] : nullptr};
  g_w3.n = n;
  return GT_OK;
}
extern "C" int gt_w3_unbind(void) {
  g_w3.n = 0;
  return GT_OK;
}

// ---- fragment-order bf16 images for the encoder layers' GEMMs (linear1.h) ------------------------------------------------
// 0 when the (rows, contraction) GEMM is not covered by the weight-stationary kernel (rows % 64, contraction % 128, <= 1024)
extern "C" size_t gt_w1_image_bytes(int64_t rows, int64_t contraction) {
  return (w1_pick_ntw(rows, contraction) || w2_covered(rows, contraction)) ? w1_image_bytes(rows, contraction) : 0;
}
// Job i as gt_w3_images: weight[i] = fp32 [N[i]][K[i]]; transposed[i] == 0 -> image of W (rows N, contraction K), != 0 -> image of W^T;
// image[i] has gt_w1_image_bytes(rows, contraction) bytes (non-zero), 16-byte aligned.
extern "C" int gt_w1_images(int n, const float* const* weight, const int64_t* N, const int64_t* K, const int* transposed,
                            void* const* image, gt_stream_t stream_) {
  GT_CHECK_ARG(n >= 0 && (n == 0 || (weight && N && K && transposed && image)), "bad arguments");
  for (int i0 = 0; i0 < n; i0 += W1_MAX_JOBS) {
    W1Jobs jobs{};
    int blocks = 0;
    const int cnt = n - i0 < W1_MAX_JOBS ? n - i0 : W1_MAX_JOBS;
    for (int i = 0; i < cnt; ++i) {
      const int s = i0 + i;
      GT_CHECK_ARG(weight[s] && image[s] && N[s] > 0 && K[s] > 0 && ((uintptr_t)image[s] & 15) == 0, "null / unaligned buffer");
      const int64_t rows = transposed[s] ? K[s] : N[s], contr = transposed[s] ? N[s] : K[s];
      GT_CHECK_ARG(w1_pick_ntw(rows, contr) != 0 || w2_covered(rows, contr), "shape not covered (gt_w1_image_bytes == 0)");
      W1Job& J = jobs.j[i];
      J.w = weight[s]; J.img = (unsigned char*)image[s]; J.R = (int)rows; J.C = (int)contr; J.ldw = (int)K[s];
      J.transposed = transposed[s] ? 1 : 0; J.block0 = blocks;
      blocks += (int)gt_cdiv((rows / 16) * (contr / 32), 4);
    }
    jobs.n = cnt;
    hipLaunchKernelGGL(k_w1_image, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, jobs);
  }
  GT_CHECK_LAUNCH();
  return GT_OK;
}
// Binds images for the calling HOST THREAD: until gt_w1_unbind(), gt_linear_fwd* / gt_linear_bwd* calls with bf16 rows in and out,
// bf16 compute, one group, no GELU and a weight (pointer, N, K) in the table run the weight-stationary kernel (forward: image_fwd[i];
// dX: image_t[i], when the call has no gate on dY; NULL keeps the tiled kernel for that direction).  Images must be current.
extern "C" int gt_w1_bind(int n, const float* const* weight, const int64_t* N, const int64_t* K, const void* const* image_fwd,
                          const void* const* image_t) {
  GT_CHECK_ARG(n >= 0 && n <= W1_MAX_BOUND && (n == 0 || (weight && N && K)), "at most 64 bound weights");
  for (int i = 0; i < n; ++i)
    g_w1.e[i] = W1Bound{weight[i], N[i], K[i], image_fwd ? image_fwd[i] : nullptr, image_t ? image_t[i] : nullptr};
  g_w1.n = n;
  return GT_OK;
}
extern "C" int gt_w1_unbind(void) {
  g_w1.n = 0;
  return GT_OK;
}
// the gate (dropout_p >= 0: the forward output of the layer BELOW; < 0: a saved multiplier) applies to the dX OUTPUT, dY is used as it is
extern "C" int gt_linear_bwd_gate_out_ok(int x_dtype, int y_dtype, int compute, const float* weight, int64_t M, int64_t N, int64_t K) {
  return (x_dtype == GT_BF16 && y_dtype == GT_BF16 && compute == GT_BF16 && M >= W1_MIN_M && w1_lookup(weight, N, K, true) &&
          w1_pick_ntw(K, N)) ? 1 : 0;
}
extern "C" int gt_linear_bwd_gate_out(int x_dtype, int y_dtype, int compute, const void* x, const float* weight, const void* dy,
                                      const void* y_or_mul, const void* dx_add1, const void* dx_add2, void* dx, float* dweight,
                                      float* dbias, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldy, float dropout_p,
                                      void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  GT_CHECK_ARG(y_or_mul && dx, "gt_linear_bwd_gate_out needs the gate tensor and dx");
  LinBwd c{x_dtype, y_dtype, compute, x, weight, dy, y_or_mul, dx_add1, dx_add2, dx, dweight, dbias, M, N, K, ldx, ldy, 1, 0, 0,
               dropout_p < 0.f ? 0.f : dropout_p, workspace, workspace_bytes, (hipStream_t)stream_};
  take_bwd(c);
  c.gate_out = true;
  c.mul_mask = dropout_p < 0.f;
  return lin_bwd(c);
}

// y = LayerNorm(resid + dropout(a)) * ln_w + ln_b with a = x W^T + b, as ONE launch: the GEMM's epilogue holds whole rows (N = the
// LayerNorm dim in one column block), saves a (the LayerNorm backward re-reads it), mean and rstd exactly as gt_linear_fwd followed by
// gt_layernorm_fwd(a, resid, ...) would (post-norm nn.TransformerEncoderLayer: x = norm1(x + dropout1(sa)), x = norm2(x + dropout2(ff));
// modules/transformer_encoder.py:28-32).  Only on the weight-stationary path: gt_linear_layernorm_fwd_ok says so (callers fall back to
// the two calls).
extern "C" int gt_linear_layernorm_fwd_ok(int dtype, int compute, const float* weight, int64_t M, int64_t N, int64_t K) {
  return (dtype == GT_BF16 && compute == GT_BF16 && M >= W1_MIN_M && w1_ln_covered(N, K) && w1_lookup(weight, N, K, false)) ? 1 : 0;
}
extern "C" int gt_linear_layernorm_fwd(int dtype, int compute, const void* x, const float* weight, const float* bias, void* a_out,
                                       int64_t M, int64_t N, int64_t K, const void* resid, const float* ln_weight, const float* ln_bias,
                                       float eps, float dropout_p, uint64_t seed, void* y, float* save_mean, float* save_rstd,
                                       gt_stream_t stream_) {
  GT_CHECK_ARG(x && weight && a_out && ln_weight && ln_bias && y && save_mean && save_rstd, "null buffer");
  GT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p must be in [0,1)");
  if (!gt_linear_layernorm_fwd_ok(dtype, compute, weight, M, N, K)) {
    gt_set_error("gt_linear_layernorm_fwd: not covered (ask gt_linear_layernorm_fwd_ok)");
    return GT_ERR_UNSUPPORTED;
  }
  if (M == 0) return GT_OK;
  hipStream_t stream = (hipStream_t)stream_;
  LinArgs d{};
  fill_drop(d, dropout_p, seed);
  L1Args l{};
  l.a = (const gt_bf16*)x; l.img = (const unsigned char*)w1_lookup(weight, N, K, false); l.bias = bias; l.out = (gt_bf16*)a_out;
  l.M = M; l.lda = K; l.ldo = N; l.N = (int)N; l.K = (int)K;
  l.ln_resid = (const gt_bf16*)resid; l.ln_w = ln_weight; l.ln_b = ln_bias; l.ln_out = (gt_bf16*)y; l.ln_mean = save_mean; l.ln_rstd = save_rstd;
  l.ln_eps = eps; l.ln_inv_keep = d.inv_keep; l.ln_thr = d.thr; l.ln_s0 = d.s0; l.ln_s1 = d.s1;
  bool ok;
  {
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin1[fwd+ln]", stream, {M, N, K, dtype, dtype, compute});
    ok = w1_launch(stream, l);
  }
  if (!ok) { gt_set_error("gt_linear_layernorm_fwd: launch set-up failed"); return GT_ERR_LAUNCH; }
  GT_CHECK_LAUNCH();
  return GT_OK;
}

// dX of a Linear whose OUTPUT gradient is at once the gradient of the LayerNorm below it (post-norm nn.TransformerEncoderLayer backward,
// modules/transformer_encoder.py:28-32: linear1's dX + the residual gradient -> norm1's backward; in_proj's dX + the residual gradient
// -> the previous layer's norm2): g = dY W (+ add1 + add2) never reaches memory, the GEMM's epilogue holds whole rows and runs
// gt_layernorm_bwd's arithmetic on them -- d_sub = d(sub-layer output), d_resid = d(residual branch), and the LayerNorm's weight / bias
// gradient through block partials in `workspace` (or the open deferred-reduce section).  weight [N][K], K = the LayerNorm dim.
// Only on the weight-stationary path: gt_linear_bwd_dx_layernorm_ok says so (callers fall back to gt_linear_bwd + gt_layernorm_bwd).
extern "C" int gt_linear_bwd_dx_layernorm_ok(int dtype, int compute, const float* weight, int64_t M, int64_t N, int64_t K) {
  return (dtype == GT_BF16 && compute == GT_BF16 && M >= W1_MIN_M && w1_lnb_covered(K, N) && w1_lookup(weight, N, K, true)) ? 1 : 0;
}
extern "C" size_t gt_linear_bwd_dx_layernorm_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  return (size_t)w1_grid_blocks(M, K, N) * 2 * (size_t)K * sizeof(float) + 256;
}
extern "C" int gt_linear_bwd_dx_layernorm(int dtype, int compute, const float* weight, const void* dy, const void* dx_add1, const void* dx_add2,
                                          int64_t M, int64_t N, int64_t K, const void* ln_x, const void* ln_resid, const float* ln_weight,
                                          const float* save_mean, const float* save_rstd, float dropout_p, uint64_t seed, void* d_sub,
                                          void* d_resid, float* ln_dweight, float* ln_dbias, void* workspace, size_t workspace_bytes,
                                          gt_stream_t stream_) {
  GT_CHECK_ARG(weight && dy && ln_x && ln_weight && save_mean && save_rstd && ln_dweight && ln_dbias, "null buffer");
  GT_CHECK_ARG(d_sub || d_resid, "nothing to compute");
  GT_CHECK_ARG(dropout_p >= 0.f && dropout_p < 1.f, "dropout_p must be in [0,1)");
  if (!gt_linear_bwd_dx_layernorm_ok(dtype, compute, weight, M, N, K)) {
    gt_set_error("gt_linear_bwd_dx_layernorm: not covered (ask gt_linear_bwd_dx_layernorm_ok)");
    return GT_ERR_UNSUPPORTED;
  }
  if (M == 0) {
    (void)hipMemsetAsync(ln_dweight, 0, (size_t)K * sizeof(float), (hipStream_t)stream_);
    (void)hipMemsetAsync(ln_dbias, 0, (size_t)K * sizeof(float), (hipStream_t)stream_);
    return GT_OK;
  }
  hipStream_t stream = (hipStream_t)stream_;
  const int blocks = w1_grid_blocks(M, K, N);
  const size_t pbytes = (size_t)blocks * 2 * (size_t)K * sizeof(float);
  float* part = (float*)gt_defer_take(pbytes);   // inside a deferred-reduce section: the column sums join its one launch
  const bool deferred = part != nullptr;
  if (!deferred) {
    if (!workspace || workspace_bytes < pbytes) { gt_set_error("gt_linear_bwd_dx_layernorm: workspace too small"); return GT_ERR_WORKSPACE; }
    if (g_dw.active && stream == g_dw.main) dw_release(workspace, workspace_bytes);   // a forked GEMM may still read partials there
    part = (float*)workspace;
  }
  LinArgs d{};
  fill_drop(d, dropout_p, seed);
  L1Args l{};
  l.a = (const gt_bf16*)dy; l.img = (const unsigned char*)w1_lookup(weight, N, K, true);
  l.add1 = (const gt_bf16*)dx_add1; l.add2 = (const gt_bf16*)dx_add2;
  l.M = M; l.lda = N; l.ldo = K; l.N = (int)K; l.K = (int)N;
  l.lnb_x = (const gt_bf16*)ln_x; l.ln_resid = (const gt_bf16*)ln_resid; l.ln_w = ln_weight;
  l.ln_mean = const_cast<float*>(save_mean); l.ln_rstd = const_cast<float*>(save_rstd);
  l.ln_inv_keep = d.inv_keep; l.ln_thr = d.thr; l.ln_s0 = d.s0; l.ln_s1 = d.s1;
  l.lnb_dsub = (gt_bf16*)d_sub; l.lnb_dresid = (gt_bf16*)d_resid; l.lnb_part = part;
  bool ok;
  {
    GtProfScope pk__(GT_PROF_GEMM_KERNEL, "k_lin1[dx+lnb]", stream, {M, N, K, dtype, dtype, compute});
    ok = w1_launch(stream, l);
  }
  if (!ok) { gt_set_error("gt_linear_bwd_dx_layernorm: launch set-up failed"); return GT_ERR_LAUNCH; }
  GT_CHECK_LAUNCH();
  if (deferred) return gt_defer_push(part, blocks, K, 2 * K, ln_dweight, part + K, K, 2 * K, ln_dbias);
  return gt_layernorm_bwd_finish(part, blocks, K, ln_dweight, ln_dbias, stream_);
}

// ---- overlap section -------------------------------------------------------------------------------
extern "C" int gt_defer_begin(void* arena, size_t bytes) {
  g_defer.active = arena && bytes > 0;
  g_defer.arena = (char*)arena;
  g_defer.cap = bytes;
  g_defer.used = 0;
  g_defer.max_take = 0;
  g_defer.jobs.n = 0;
  g_defer.blocks = 0;
  return GT_OK;
}
// Only partial buffers of at most `max_take_bytes` join the open section (0 = every size): the big batches keep the weight-gradient
// GEMMs' immediate reduces (their partials stay in the reused, cache-resident workspaces) and defer the LayerNorms' column sums
extern "C" int gt_defer_limit(size_t max_take_bytes) {
  g_defer.max_take = max_take_bytes;
  return GT_OK;
}
extern "C" void* gt_defer_take(size_t bytes) {
  if (!g_defer.active || g_defer.jobs.n >= DEFER_MAX_JOBS || (g_defer.max_take && bytes > g_defer.max_take)) return nullptr;
  const size_t need = (bytes + 255) & ~(size_t)255;
  if (g_defer.used + need > g_defer.cap) return nullptr;
  void* p = g_defer.arena + g_defer.used;
  g_defer.used += need;
  return p;
}
extern "C" int gt_defer_room(int jobs) { return (g_defer.active && g_defer.jobs.n + jobs <= DEFER_MAX_JOBS) ? 1 : 0; }
extern "C" int gt_defer_push_strided(const float* part, int nparts, int64_t len, int64_t stride, float* out, int64_t ostride) {
  GT_CHECK_ARG(ostride >= 1, "bad output stride");
  const int rc = gt_defer_push(part, nparts, len, stride, out, nullptr, 0, 0, nullptr);
  if (rc) return rc;
  g_defer.jobs.j[g_defer.jobs.n - 1].ostride = ostride;
  return GT_OK;
}
extern "C" int gt_defer_push(const float* part, int nparts, int64_t len, int64_t stride, float* out, const float* part2, int64_t len2,
                             int64_t stride2, float* out2) {
  GT_CHECK_ARG(g_defer.active && g_defer.jobs.n < DEFER_MAX_JOBS, "no open section / job list full (a gt_defer_take came first?)");
  GT_CHECK_ARG(part && out && nparts >= 1 && len > 0 && (len2 == 0 || (part2 && out2)), "bad job");
  DeferJob& q = g_defer.jobs.j[g_defer.jobs.n++];
  q.part = part; q.part2 = len2 ? part2 : nullptr; q.out = out; q.out2 = len2 ? out2 : nullptr;
  q.len = len; q.len2 = len2; q.stride = stride; q.stride2 = stride2; q.nparts = nparts; q.ostride = 1;
  q.block0 = g_defer.blocks;
  const int64_t nb = gt_cdiv(len + len2, 256);
  g_defer.blocks += (int)(nb < 512 ? nb : 512);
  return GT_OK;
}
extern "C" int gt_defer_flush(gt_stream_t stream_) {
  if (!g_defer.active || g_defer.jobs.n == 0) return GT_OK;
  hipLaunchKernelGGL(k_defer_reduce, dim3((unsigned)g_defer.blocks), dim3(256), 0, (hipStream_t)stream_, g_defer.jobs);
  g_defer.jobs.n = 0;
  g_defer.blocks = 0;
  GT_CHECK_LAUNCH();
  return GT_OK;
}
extern "C" int gt_defer_end(void) {
  GT_CHECK_ARG(!g_defer.active || g_defer.jobs.n == 0, "queued sums were never flushed");
  g_defer.active = false;
  return GT_OK;
}

extern "C" int gt_overlap_dw_begin(gt_stream_t main_, gt_stream_t side_) {
  GT_CHECK_ARG(side_ && main_ != side_, "need a distinct side stream");
  if (!g_dw.ev_fork) {
    if (hipEventCreateWithFlags(&g_dw.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&g_dw.ev_join, hipEventDisableTiming) != hipSuccess) {
      gt_set_error("gt_overlap_dw_begin: event creation failed");
      return GT_ERR_LAUNCH;
    }
    for (int i = 0; i < DW_RING; ++i)
      if (hipEventCreateWithFlags(&g_dw.ring[i].ev, hipEventDisableTiming) != hipSuccess) {
        gt_set_error("gt_overlap_dw_begin: event creation failed");
        return GT_ERR_LAUNCH;
      }
  }
  g_dw.main = (hipStream_t)main_;
  g_dw.side = (hipStream_t)side_;
  g_dw.active = true;
  g_dw.urgent = false;
  g_dw.n = 0;
  return GT_OK;
}
extern "C" int gt_overlap_dw_sync(void) {
  if (!g_dw.active) return GT_OK;
  dw_join_all();
  return GT_OK;
}
// For the other entry points whose LAST launch only produces parameter gradients (the column finish of a LayerNorm backward,
// the partial reduce of an aggregate backward): inside an overlap section on the section's main stream, returns the overlap
// stream after ordering it behind everything queued on `stream` so far; otherwise `stream` itself.  A launch that went to the
// overlap stream is then booked with gt_overlap_dw_booked(workspace it reads, bytes) so that gt_overlap_dw_release covers it.
extern "C" gt_stream_t gt_overlap_dw_fork(gt_stream_t stream, unsigned prof_category) {
  // (not while the launch profiler brackets the caller's category: its events sit on the caller's stream only)
  if (!g_dw.active || (hipStream_t)stream != g_dw.main || (gt_prof_mask() & prof_category)) return stream;
  (void)hipEventRecord(g_dw.ev_fork, g_dw.main);
  (void)hipStreamWaitEvent(g_dw.side, g_dw.ev_fork, 0);
  return (gt_stream_t)g_dw.side;
}
extern "C" void gt_overlap_dw_booked(const void* workspace, size_t bytes) {
  if (g_dw.active) dw_forked(workspace, bytes);
}
extern "C" int gt_overlap_dw_urgent(int on) {
  g_dw.urgent = on != 0;
  return GT_OK;
}
extern "C" int gt_overlap_dw_release(const void* workspace, size_t bytes) {
  dw_release(workspace, bytes);
  return GT_OK;
}
extern "C" int gt_overlap_dw_end(void) {
  const int rc = gt_overlap_dw_sync();
  g_dw.active = false;
  return rc;
}
