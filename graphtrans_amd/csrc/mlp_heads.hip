// mlp_heads.hip -- the prediction heads of the PNA baseline (gt_head_group_* and gt_head_mlp_*).
//
// Reference semantics (paths under the reference tree): models/pna.py:53-71, :99-104
//   max_seq_len = L  : per position  Linear(D, D) -> ReLU -> Linear(D, T).  The hidden layers stack into one (B, D) x (D, L*D) GEMM
//                      (gt_linear_fwd, ReLU epilogue); the OUTPUT layers are L different (B, D) x (D, T) products into the one logits
//                      buffer [B][c4(L*T)] -- gt_head_group_*: the group-tiled generalisation of k_heads_fwd / k_heads_dx (linear_heads.h).
//   max_seq_len None : mlp = Linear(D, 35) -> ReLU -> Linear(35, 17) -> ReLU -> Linear(17, T) -- gt_head_mlp_*: plain fp32 FMA, the
//                      widths 35 / 17 fit no MFMA tile and no 16-byte row.
//
// Grouped layer, the hazard: head g's first column g*T is only 4-byte aligned (T = 5002) and a 16-column tile must not straddle two
// groups (the H slab depends on the group).  So the grid is (column block WITHIN the group, group, ...), every Y store and every bias /
// dY load is a scalar access at its true address, and the columns [G*T, ldy) are never touched.  H and W rows stay 16-byte aligned
// (ldh % 4 == 0, K % 16 == 0).
//   forward : block = 256 rows x 128 columns of one group, 8 waves of 64 x 64 (16 accumulator tiles), operands straight from global / L2.
//   dH      : contraction over T in 32-deep steps; block = a step range x all rows x a 128-wide chunk of K, W slab through LDS; fp32
//             partials [G][nblk][M][K], one fixed-order reduce that also applies the ReLU mask.
//   dW, db  : contraction over the M rows (no split): block = 64 columns x 64 k of one group, both operands through LDS (read
//             transposed); the k-chunk 0 blocks add the column sums of their dY tiles = dbias.
// No atomics anywhere, every sum in a fixed order: two runs give the same bits.
#include "gt_common.h"
#include "mfma_frag.h"

namespace {
using namespace gtf;

struct HgArgs {
  const float* h;      // [M][ldh]: group g reads columns [g*K, (g+1)*K)
  const float* w;      // [G*T][K]
  const float* bias;   // fwd: [G*T] or null
  const float* dy;     // bwd: dY [M][ldy]
  float* out;          // fwd: Y [M][ldy]; dH: partials [G][nblk][M][K]; dW: dW [G*T][K]
  float* db;           // dW: dbias [G*T] or null
  int64_t M, ldh, ldy;
  int G, K, T;
  int nblk, steps, kch;   // dH: blocks along T, 32-deep steps of T, 128-wide chunks of K
};
constexpr int HG_LDW = 128 + 4;   // LDS row pitch of a W slab (k_heads_dx)
constexpr int HG_LDT = 64 + 4;    // LDS row pitch of the dW tiles

// 4 x 4 tile products of one 32-deep step (heads_mma of linear_heads.h): fp32 slot by slot over the 16 independent accumulators
__device__ __forceinline__ void hg_mma(const Frag<float> (&fa)[4], const Frag<float> (&fb)[4], f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j].v[e], fb[i].v[e], acc[i][j], 0, 0, 0);
}
__device__ __forceinline__ void hg_mma(const Frag<gt_bf16> (&fa)[4], const Frag<gt_bf16> (&fb)[4], f32x4 (&acc)[4][4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][j] = mma(fa[j], fb[i], acc[i][j]);
}

// grid (column blocks of 128 within a group, G, row blocks of 256)
template <typename TC>
__global__ void __launch_bounds__(512) k_hg_fwd(HgArgs a) {
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6, wm = wv >> 1, wk = wv & 1;
  const int grp = blockIdx.y;
  const int64_t m0 = (int64_t)blockIdx.z * 256 + wm * 64;
  const int c0 = blockIdx.x * 128 + wk * 64;   // column inside the group
  if (m0 >= a.M || c0 >= a.T) return;          // (wave-uniform; this kernel has no barrier)
  const float* xr[4];
  const float* wr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = m0 + i * 16 + n;
    const int col = c0 + i * 16 + n;
    xr[i] = a.h + (row < a.M ? row : a.M - 1) * a.ldh + (int64_t)grp * a.K + g * 8;   // clamped rows / columns are computed, never stored
    wr[i] = a.w + ((int64_t)grp * a.T + (col < a.T ? col : a.T - 1)) * a.K + g * 8;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s * 32 < a.K; ++s) {
    const bool live = s * 32 + g * 8 < a.K;   // K % 16 == 0: the last step of K % 32 == 16 has two zero lane groups
    Frag<TC> fx[4], fw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t[8];
      const float4 x0 = live ? *reinterpret_cast<const float4*>(xr[i] + s * 32) : gt_zero4();
      const float4 x1 = live ? *reinterpret_cast<const float4*>(xr[i] + s * 32 + 4) : gt_zero4();
      t[0] = x0.x; t[1] = x0.y; t[2] = x0.z; t[3] = x0.w; t[4] = x1.x; t[5] = x1.y; t[6] = x1.z; t[7] = x1.w;
      fx[i] = frag_from_f32<TC>(t);
      const float4 w0 = live ? *reinterpret_cast<const float4*>(wr[i] + s * 32) : gt_zero4();
      const float4 w1 = live ? *reinterpret_cast<const float4*>(wr[i] + s * 32 + 4) : gt_zero4();
      t[0] = w0.x; t[1] = w0.y; t[2] = w0.z; t[3] = w0.w; t[4] = w1.x; t[5] = w1.y; t[6] = w1.z; t[7] = w1.w;
      fw[i] = frag_from_f32<TC>(t);
    }
    hg_mma(fw, fx, acc);   // c[r] = Y[m0 + i*16 + n][group column c0 + j*16 + g*4 + r]
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = m0 + i * 16 + n;
    if (row >= a.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = c0 + j * 16 + g * 4;
      const int64_t gc = (int64_t)grp * a.T + col;   // only 4-byte aligned: scalar stores
      float* o = a.out + row * a.ldy + gc;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (col + e < a.T) o[e] = acc[i][j][e] + (a.bias ? a.bias[gc + e] : 0.f);
    }
  }
}

// grid (nblk step ranges of T, row blocks of 256, G * kch)
template <typename TC>
__global__ void __launch_bounds__(512) k_hg_dx(HgArgs a) {
  __shared__ __attribute__((aligned(16))) float sw[2][32 * HG_LDW];
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6, wm = wv >> 1, wk = wv & 1;
  const int b = blockIdx.x;
  const int grp = blockIdx.z / a.kch, kbase = (blockIdx.z % a.kch) * 128;
  const int s_lo = (int)((int64_t)b * a.steps / a.nblk), s_hi = (int)((int64_t)(b + 1) * a.steps / a.nblk);
  const int64_t m0 = (int64_t)blockIdx.y * 256 + wm * 64;
  const float* zr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = m0 + i * 16 + n;
    zr[i] = a.dy + (row < a.M ? row : a.M - 1) * a.ldy + (int64_t)grp * a.T;
  }
  const float* wg = a.w + (int64_t)grp * a.T * a.K;
  // staging of a W slab (32 rows of the group x 128 of K): thread -> 2 x 16 bytes, rows sr0 / sr1, 16-byte column sc
  const int sr0 = threadIdx.x >> 5, sr1 = sr0 + 16, sc = (threadIdx.x & 31) * 4;
  const bool kin = kbase + sc < a.K;   // (K % 4 == 0: the 16 bytes are inside or outside as a whole)
  auto slab = [&](int s, float4& w0, float4& w1) {
    const int r0 = s * 32 + sr0, r1 = s * 32 + sr1;
    w0 = kin && r0 < a.T ? *reinterpret_cast<const float4*>(wg + (int64_t)r0 * a.K + kbase + sc) : gt_zero4();
    w1 = kin && r1 < a.T ? *reinterpret_cast<const float4*>(wg + (int64_t)r1 * a.K + kbase + sc) : gt_zero4();
  };
  float4 w0, w1;
  slab(s_lo, w0, w1);
  *reinterpret_cast<float4*>(&sw[0][sr0 * HG_LDW + sc]) = w0;
  *reinterpret_cast<float4*>(&sw[0][sr1 * HG_LDW + sc]) = w1;
  __syncthreads();
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = s_lo; s < s_hi; ++s) {
    const int cur = (s - s_lo) & 1;
    slab(s + 1 < s_hi ? s + 1 : s, w0, w1);   // the next slab (the last iteration reloads its own) while this one is multiplied
    Frag<TC> fz[4], fw[4];
    const int c = s * 32 + g * 8;   // this lane's 8 columns of the group: 4-byte aligned addresses, zero beyond T
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = c + e < a.T ? zr[i][c + e] : 0.f;
      fz[i] = frag_from_f32<TC>(t);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = sw[cur][(g * 8 + e) * HG_LDW + wk * 64 + j * 16 + n];
      fw[j] = frag_from_f32<TC>(t);
    }
    hg_mma(fw, fz, acc);   // c[r] = dH[m0 + i*16 + n][kbase + wk*64 + j*16 + g*4 + r]
    *reinterpret_cast<float4*>(&sw[cur ^ 1][sr0 * HG_LDW + sc]) = w0;
    *reinterpret_cast<float4*>(&sw[cur ^ 1][sr1 * HG_LDW + sc]) = w1;
    __syncthreads();
  }
  float* part = a.out + ((int64_t)grp * a.nblk + b) * a.M * a.K;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = m0 + i * 16 + n;
    if (row >= a.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = kbase + wk * 64 + j * 16 + g * 4;
      if (col < a.K) *reinterpret_cast<float4*>(part + row * a.K + col) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

// dH[m][g*K + k] = [H > 0] * sum over the step-range blocks, in block order.  grid (M, G), a thread per 16-byte column
__global__ void __launch_bounds__(128) k_hg_dx_reduce(const float* __restrict__ part, int nblk, int64_t M, int K, const float* __restrict__ h,
                                                      int64_t ldh, int relu, float* __restrict__ dh, int64_t lddh) {
  const int64_t m = blockIdx.x;
  const int grp = blockIdx.y;
  const float* p = part + ((int64_t)grp * nblk * M + m) * K;
  const int64_t bs = M * K;
  for (int c = threadIdx.x * 4; c < K; c += 128 * 4) {
    float4 t = gt_zero4();
    int b = 0;
    for (; b + 4 <= nblk; b += 4) {
      float4 u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = *reinterpret_cast<const float4*>(p + (b + q) * bs + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) t = gt_add4(t, u[q]);
    }
    for (; b < nblk; ++b) t = gt_add4(t, *reinterpret_cast<const float4*>(p + b * bs + c));
    if (relu) {
      const float4 x = *reinterpret_cast<const float4*>(h + m * ldh + (int64_t)grp * K + c);
      t = make_float4(x.x > 0.f ? t.x : 0.f, x.y > 0.f ? t.y : 0.f, x.z > 0.f ? t.z : 0.f, x.w > 0.f ? t.w : 0.f);
    }
    *reinterpret_cast<float4*>(dh + m * lddh + (int64_t)grp * K + c) = t;
  }
}

// grid (column blocks of 64 within a group, k blocks of 64, G); 4 waves of 32 x 32
template <typename TC>
__global__ void __launch_bounds__(256) k_hg_dw(HgArgs a) {
  __shared__ __attribute__((aligned(16))) float sdy[32 * HG_LDT];
  __shared__ __attribute__((aligned(16))) float sh[32 * HG_LDT];
  const int lane = threadIdx.x & 63, n = lane & 15, g = lane >> 4, wv = threadIdx.x >> 6, wn = wv >> 1, wk = wv & 1;
  const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64, grp = blockIdx.z;
  const float* dyg = a.dy + (int64_t)grp * a.T + n0;
  const float* hg = a.h + (int64_t)grp * a.K + k0;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;
  const bool do_db = a.db && blockIdx.y == 0 && threadIdx.x < 64;
  for (int64_t m0 = 0; m0 < a.M; m0 += 32) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {   // dY tile [32 rows][64 columns of the group]: 4-byte aligned addresses
      const int idx = threadIdx.x + q * 256, r = idx >> 6, c = idx & 63;
      sdy[r * HG_LDT + c] = (m0 + r < a.M && n0 + c < a.T) ? dyg[(m0 + r) * a.ldy + c] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {   // H tile [32 rows][64 of K]
      const int idx = threadIdx.x + q * 256, r = idx >> 4, c = (idx & 15) * 4;
      const float4 v = (m0 + r < a.M && k0 + c < a.K) ? *reinterpret_cast<const float4*>(hg + (m0 + r) * a.ldh + c) : gt_zero4();
      *reinterpret_cast<float4*>(&sh[r * HG_LDT + c]) = v;
    }
    __syncthreads();
    if (do_db)
#pragma unroll
      for (int r = 0; r < 32; ++r) dbacc += sdy[r * HG_LDT + threadIdx.x];   // rows ascend: a fixed order
    Frag<TC> fa[2], fb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float t[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = sdy[(g * 8 + e) * HG_LDT + wn * 32 + i * 16 + n];
      fa[i] = frag_from_f32<TC>(t);
#pragma unroll
      for (int e = 0; e < 8; ++e) t[e] = sh[(g * 8 + e) * HG_LDT + wk * 32 + i * 16 + n];
      fb[i] = frag_from_f32<TC>(t);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = mma(fa[i], fb[j], acc[i][j]);   // c[r] = dW[n0 + wn*32 + i*16 + g*4 + r][k0 + wk*32 + j*16 + n]
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + wk * 32 + j * 16 + n;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n0 + wn * 32 + i * 16 + g * 4 + r;
        if (nn < a.T && kk < a.K) a.out[((int64_t)grp * a.T + nn) * a.K + kk] = acc[i][j][r];
      }
    }
  if (do_db && n0 + (int)threadIdx.x < a.T) a.db[(int64_t)grp * a.T + n0 + threadIdx.x] = dbacc;
}

// ---- the narrow MLP head -------------------------------------------------------------------------------------------------------
// 16 rows per block, 256 threads: thread (r = tid >> 4, q = tid & 15) owns the outputs q, q + 16, q + 32, q + 48 of row r.
constexpr int MH_R = 16;      // rows per block
constexpr int MH_W = 64;      // the widest hidden layer; also the chunk of D staged at a time
constexpr int MH_LD = MH_W + 1;

struct MlpArgs {
  const float *x, *w1, *b1, *w2, *b2, *w3, *b3;
  const float *a1c, *a2c, *dy;    // bwd: the saved activations, dY [M][ldy]
  float *a1, *a2, *y;             // fwd: a1 [M][H1], a2 [M][H2], y [M][ldy];  bwd: d1 [M][H1], d2 [M][H2], dx [M][lddx]
  int64_t M, ldx, ldy, lddx;
  int D, H1, H2, T;
};

// the [<= 64][<= 64] matrix w [rows][cols] (contiguous) -> LDS image [64][MH_LD], zero filled
__device__ __forceinline__ void mh_stage(float* s, const float* w, int rows, int cols) {
  for (int idx = threadIdx.x; idx < MH_W * MH_W; idx += 256) {
    const int r = idx >> 6, c = idx & 63;
    s[r * MH_LD + c] = (r < rows && c < cols) ? w[r * cols + c] : 0.f;
  }
}

__global__ void __launch_bounds__(256) k_mlp_fwd(MlpArgs a) {
  __shared__ float sw[MH_W * MH_LD];    // a W1 chunk [h][d], then W2 [j][h]
  __shared__ float sx[MH_R * MH_LD];    // an x chunk, then a2
  __shared__ float sa[MH_R * MH_LD];    // a1
  const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * MH_R + r;
  const bool rin = row < a.M;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int dc = 0; dc < a.D; dc += MH_W) {
    {   // x chunk: 16 rows x 64 = 256 x 16 bytes
      const int c = q * 4;
      const float4 v = (rin && dc + c < a.D) ? *reinterpret_cast<const float4*>(a.x + row * a.ldx + dc + c) : gt_zero4();
      float* d = &sx[r * MH_LD + c];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // W1 chunk: 64 rows x 64 = 1024 x 16 bytes (D % 4 == 0: rows are 16-byte aligned)
      const int idx = threadIdx.x + u * 256, hr = idx >> 4, c = (idx & 15) * 4;
      const float4 v = (hr < a.H1 && dc + c < a.D) ? *reinterpret_cast<const float4*>(a.w1 + (int64_t)hr * a.D + dc + c) : gt_zero4();
      float* d = &sw[hr * MH_LD + c];
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
#pragma unroll 8
    for (int d = 0; d < MH_W; ++d) {
      const float xv = sx[r * MH_LD + d];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(xv, sw[(q + 16 * u) * MH_LD + d], acc[u]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int h = q + 16 * u;
    const float v = h < a.H1 ? fmaxf(acc[u] + a.b1[h], 0.f) : 0.f;
    sa[r * MH_LD + h] = v;
    if (rin && h < a.H1) a.a1[row * a.H1 + h] = v;
  }
  mh_stage(sw, a.w2, a.H2, a.H1);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = 0.f;
  for (int h = 0; h < a.H1; ++h) {
    const float av = sa[r * MH_LD + h];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(av, sw[(q + 16 * u) * MH_LD + h], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = q + 16 * u;
    const float v = j < a.H2 ? fmaxf(acc[u] + a.b2[j], 0.f) : 0.f;
    sx[r * MH_LD + j] = v;
    if (rin && j < a.H2) a.a2[row * a.H2 + j] = v;
  }
  __syncthreads();
  if (!rin) return;
  for (int t = q; t < a.T; t += 16) {
    const float* w = a.w3 + (int64_t)t * a.H2;
    float s = 0.f;
    for (int j = 0; j < a.H2; ++j) s = fmaf(sx[r * MH_LD + j], w[j], s);
    a.y[row * a.ldy + t] = s + a.b3[t];
  }
}

// d2 = [a2 > 0] dY W3, d1 = [a1 > 0] d2 W2 (both saved for the parameter pass), dx = d1 W1
__global__ void __launch_bounds__(256) k_mlp_bwd_rows(MlpArgs a) {
  __shared__ float sw[MH_W * MH_LD];    // W2 [j][h]
  __shared__ float s2[MH_R * MH_LD];    // d2
  __shared__ float s1[MH_R * MH_LD];    // d1
  const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * MH_R + r;
  const bool rin = row < a.M;
  const int64_t rc = rin ? row : a.M - 1;
  mh_stage(sw, a.w2, a.H2, a.H1);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* dyr = a.dy + rc * a.ldy;
  for (int t = 0; t < a.T; ++t) {
    const float dv = dyr[t];
    const float* w = a.w3 + (int64_t)t * a.H2;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = q + 16 * u;
      acc[u] = fmaf(dv, j < a.H2 ? w[j] : 0.f, acc[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int j = q + 16 * u;
    const float v = (rin && j < a.H2 && a.a2c[row * a.H2 + j] > 0.f) ? acc[u] : 0.f;
    s2[r * MH_LD + j] = v;
    if (rin && j < a.H2) a.a2[row * a.H2 + j] = v;
    acc[u] = 0.f;
  }
  __syncthreads();
  for (int j = 0; j < a.H2; ++j) {
    const float dv = s2[r * MH_LD + j];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(dv, sw[j * MH_LD + q + 16 * u], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int h = q + 16 * u;
    const float v = (rin && h < a.H1 && a.a1c[row * a.H1 + h] > 0.f) ? acc[u] : 0.f;
    s1[r * MH_LD + h] = v;
    if (rin && h < a.H1) a.a1[row * a.H1 + h] = v;
  }
  __syncthreads();
  if (!a.y) return;   // (block-uniform) no dx asked for
  const int64_t r0 = (int64_t)blockIdx.x * MH_R;
  for (int d = threadIdx.x; d < a.D; d += 256) {   // a thread per column: W1 is read once per block, d1 broadcast from LDS
    float o[MH_R];
#pragma unroll
    for (int i = 0; i < MH_R; ++i) o[i] = 0.f;
    for (int h = 0; h < a.H1; ++h) {
      const float w = a.w1[(int64_t)h * a.D + d];
#pragma unroll
      for (int i = 0; i < MH_R; ++i) o[i] = fmaf(s1[i * MH_LD + h], w, o[i]);
    }
#pragma unroll
    for (int i = 0; i < MH_R; ++i)
      if (r0 + i < a.M) a.y[(r0 + i) * a.lddx + d] = o[i];
  }
}

// the six parameter gradients: a thread per element, the M rows summed in ascending order.
//   dW1[h][d] = sum_b d1[b][h] x[b][d]    dW2[j][h] = sum_b d2[b][j] a1[b][h]    dW3[t][j] = sum_b dY[b][t] a2[b][j]    db = the left factor alone
struct MlpGradArgs {
  const float *x, *a1, *a2, *d1, *d2, *dy;
  float *dw1, *db1, *dw2, *db2, *dw3, *db3;
  int64_t M, ldx, ldy;
  int D, H1, H2, T;
};
__global__ void __launch_bounds__(256) k_mlp_bwd_params(MlpGradArgs a) {
  int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n1 = (int64_t)a.H1 * a.D, n2 = (int64_t)a.H2 * a.H1, n3 = (int64_t)a.T * a.H2;
  const float *pa, *pb = nullptr;
  int64_t sa, sb = 0;
  float* out;
  if (e < n1) { pa = a.d1 + e / a.D; sa = a.H1; pb = a.x + e % a.D; sb = a.ldx; out = a.dw1 + e; }
  else if ((e -= n1) < a.H1) { pa = a.d1 + e; sa = a.H1; out = a.db1 + e; }
  else if ((e -= a.H1) < n2) { pa = a.d2 + e / a.H1; sa = a.H2; pb = a.a1 + e % a.H1; sb = a.H1; out = a.dw2 + e; }
  else if ((e -= n2) < a.H2) { pa = a.d2 + e; sa = a.H2; out = a.db2 + e; }
  else if ((e -= a.H2) < n3) { pa = a.dy + e / a.H2; sa = a.ldy; pb = a.a2 + e % a.H2; sb = a.H2; out = a.dw3 + e; }
  else if ((e -= n3) < a.T) { pa = a.dy + e; sa = a.ldy; out = a.db3 + e; }
  else return;
  float s = 0.f;
  int64_t b = 0;
  for (; b + 4 <= a.M; b += 4) {
    float u[4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { u[i] = pa[(b + i) * sa]; v[i] = pb ? pb[(b + i) * sb] : 1.f; }
#pragma unroll
    for (int i = 0; i < 4; ++i) s = fmaf(u[i], v[i], s);
  }
  for (; b < a.M; ++b) s = fmaf(pa[b * sa], pb ? pb[b * sb] : 1.f, s);
  *out = s;
}

// ---- argument rules ---------------------------------------------------------------------------------------------------------------
int hg_check(const char* fn, int compute, int64_t M, int64_t G, int64_t K, int64_t T) {
  const int c = gt_compute_base(compute);
  if (c != GT_F32 && c != GT_BF16) { gt_set_error("%s: bad compute type", fn); return GT_ERR_INVALID_ARG; }
  if (M < 1 || M > 4096 || G < 1 || G > 16 || T < 1 || T > (1 << 24)) {
    gt_set_error("%s: 1 <= M <= 4096, 1 <= G <= 16 and 1 <= T <= 2^24 expected, got M %lld G %lld T %lld", fn, (long long)M, (long long)G, (long long)T);
    return GT_ERR_INVALID_ARG;
  }
  if (K < 16 || K % 16 != 0 || K > 512) {
    gt_set_error("%s: K = %lld must be a multiple of 16 in [16, 512]", fn, (long long)K);
    return GT_ERR_UNSUPPORTED;
  }
  return GT_OK;
}
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int hg_dx_blocks(int64_t M, int64_t G, int64_t K, int64_t T) {
  const int64_t steps = gt_cdiv(T, 32), others = G * gt_cdiv(K, 128) * gt_cdiv(M, 256);
  int64_t nb = 512 / others;
  nb = nb < 1 ? 1 : (nb > 64 ? 64 : nb);
  return (int)(nb < steps ? nb : steps);
}

int mh_check(const char* fn, int compute, int64_t M, int64_t D, int64_t H1, int64_t H2, int64_t T) {
  const int c = gt_compute_base(compute);
  if (c != GT_F32 && c != GT_BF16) { gt_set_error("%s: bad compute type", fn); return GT_ERR_INVALID_ARG; }
  if (M < 1 || M > (1 << 20) || T < 1 || T > (1 << 20)) {
    gt_set_error("%s: 1 <= M, T <= 2^20 expected, got M %lld T %lld", fn, (long long)M, (long long)T);
    return GT_ERR_INVALID_ARG;
  }
  if (D < 4 || D % 4 != 0 || D > 1024) { gt_set_error("%s: D = %lld must be a multiple of 4 in [4, 1024]", fn, (long long)D); return GT_ERR_UNSUPPORTED; }
  if (H1 < 1 || H1 > MH_W || H2 < 1 || H2 > MH_W) {
    gt_set_error("%s: hidden widths %lld, %lld must be in [1, %d]", fn, (long long)H1, (long long)H2, MH_W);
    return GT_ERR_UNSUPPORTED;
  }
  return GT_OK;
}

}  // namespace

extern "C" size_t gt_head_group_workspace_bytes(int64_t M, int64_t G, int64_t K, int64_t T) {
  if (M < 1 || G < 1 || K < 1 || T < 1) return 0;
  return (size_t)G * hg_dx_blocks(M, G, K, T) * (size_t)M * K * sizeof(float);
}

extern "C" int gt_head_group_fwd(int compute, const float* h, int64_t ldh, const float* w, const float* bias, float* y, int64_t ldy, int64_t M,
                                 int64_t G, int64_t K, int64_t T, gt_stream_t stream_) {
  int rc = hg_check("gt_head_group_fwd", compute, M, G, K, T);
  if (rc) return rc;
  GT_CHECK_ARG(h && w && y, "null buffer");
  GT_CHECK_ARG(ldh >= G * K && ldh % 4 == 0, "ldh must be a multiple of 4 and at least G * K");
  GT_CHECK_ARG(ldy >= G * T && ldy % 4 == 0, "ldy must be a multiple of 4 and at least G * T");
  GT_CHECK_ARG(al16(h) && al16(w), "h and w must be 16-byte aligned");
  HgArgs a{};
  a.h = h; a.w = w; a.bias = bias; a.out = y;
  a.M = M; a.ldh = ldh; a.ldy = ldy; a.G = (int)G; a.K = (int)K; a.T = (int)T;
  GtProfScope prof(GT_PROF_LINEAR, "head_group_fwd", stream_, {M, G, K, T});
  const dim3 grid((unsigned)gt_cdiv(T, 128), (unsigned)G, (unsigned)gt_cdiv(M, 256));
  hipStream_t stream = (hipStream_t)stream_;
  if (gt_compute_base(compute) == GT_F32) hipLaunchKernelGGL(k_hg_fwd<float>, grid, dim3(512), 0, stream, a);
  else hipLaunchKernelGGL(k_hg_fwd<gt_bf16>, grid, dim3(512), 0, stream, a);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_head_group_bwd(int compute, const float* h, int64_t ldh, const float* w, const float* dy, int64_t lddy, int relu_mask,
                                 float* dh, int64_t lddh, float* dw, float* dbias, int64_t M, int64_t G, int64_t K, int64_t T,
                                 void* workspace, size_t workspace_bytes, gt_stream_t stream_) {
  int rc = hg_check("gt_head_group_bwd", compute, M, G, K, T);
  if (rc) return rc;
  GT_CHECK_ARG(h && w && dy, "null buffer");
  GT_CHECK_ARG(ldh >= G * K && ldh % 4 == 0, "ldh must be a multiple of 4 and at least G * K");
  GT_CHECK_ARG(lddy >= G * T && lddy % 4 == 0, "lddy must be a multiple of 4 and at least G * T");
  GT_CHECK_ARG(!dh || (lddh >= G * K && lddh % 4 == 0), "lddh must be a multiple of 4 and at least G * K");
  GT_CHECK_ARG(al16(h) && al16(w) && al16(dh), "h, w and dh must be 16-byte aligned");
  GT_CHECK_ARG(dw || !dbias, "dbias is computed beside dw");
  hipStream_t stream = (hipStream_t)stream_;
  const bool f32 = gt_compute_base(compute) == GT_F32;
  HgArgs a{};
  a.h = h; a.w = w; a.dy = dy;
  a.M = M; a.ldh = ldh; a.ldy = lddy; a.G = (int)G; a.K = (int)K; a.T = (int)T;
  GtProfScope prof(GT_PROF_LINEAR, "head_group_bwd", stream_, {M, G, K, T});
  if (dh) {
    if (!workspace || !al16(workspace) || workspace_bytes < gt_head_group_workspace_bytes(M, G, K, T)) {
      gt_set_error("gt_head_group_bwd: a 16-byte aligned workspace of %zu bytes is needed", gt_head_group_workspace_bytes(M, G, K, T));
      return GT_ERR_WORKSPACE;
    }
    a.out = (float*)workspace;
    a.steps = (int)gt_cdiv(T, 32);
    a.nblk = hg_dx_blocks(M, G, K, T);
    a.kch = (int)gt_cdiv(K, 128);
    const dim3 grid((unsigned)a.nblk, (unsigned)gt_cdiv(M, 256), (unsigned)(G * a.kch));
    if (f32) hipLaunchKernelGGL(k_hg_dx<float>, grid, dim3(512), 0, stream, a);
    else hipLaunchKernelGGL(k_hg_dx<gt_bf16>, grid, dim3(512), 0, stream, a);
    hipLaunchKernelGGL(k_hg_dx_reduce, dim3((unsigned)M, (unsigned)G), dim3(128), 0, stream, (const float*)workspace, a.nblk, M, (int)K, h, ldh,
                       relu_mask ? 1 : 0, dh, lddh);
  }
  if (dw) {
    a.out = dw;
    a.db = dbias;
    const dim3 grid((unsigned)gt_cdiv(T, 64), (unsigned)gt_cdiv(K, 64), (unsigned)G);
    if (f32) hipLaunchKernelGGL(k_hg_dw<float>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(k_hg_dw<gt_bf16>, grid, dim3(256), 0, stream, a);
  }
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" size_t gt_head_mlp_workspace_bytes(int64_t M, int64_t H1, int64_t H2) {
  if (M < 1 || H1 < 1 || H2 < 1) return 0;
  return (size_t)M * (size_t)(H1 + H2) * sizeof(float);
}

extern "C" int gt_head_mlp_fwd(int compute, const float* x, int64_t ldx, const float* w1, const float* b1, const float* w2, const float* b2,
                               const float* w3, const float* b3, float* a1, float* a2, float* y, int64_t ldy, int64_t M, int64_t D,
                               int64_t H1, int64_t H2, int64_t T, gt_stream_t stream_) {
  int rc = mh_check("gt_head_mlp_fwd", compute, M, D, H1, H2, T);
  if (rc) return rc;
  GT_CHECK_ARG(x && w1 && b1 && w2 && b2 && w3 && b3 && a1 && a2 && y, "null buffer");
  GT_CHECK_ARG(ldx >= D && ldx % 4 == 0, "ldx must be a multiple of 4 and at least D");
  GT_CHECK_ARG(ldy >= T, "ldy must be at least T");
  GT_CHECK_ARG(al16(x) && al16(w1), "x and w1 must be 16-byte aligned");
  MlpArgs a{};
  a.x = x; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.a1 = a1; a.a2 = a2; a.y = y;
  a.M = M; a.ldx = ldx; a.ldy = ldy; a.D = (int)D; a.H1 = (int)H1; a.H2 = (int)H2; a.T = (int)T;
  GtProfScope prof(GT_PROF_LINEAR, "head_mlp_fwd", stream_, {M, D, H1, H2, T});
  hipLaunchKernelGGL(k_mlp_fwd, dim3((unsigned)gt_cdiv(M, MH_R)), dim3(256), 0, (hipStream_t)stream_, a);
  GT_CHECK_LAUNCH();
  return GT_OK;
}

extern "C" int gt_head_mlp_bwd(int compute, const float* x, int64_t ldx, const float* w1, const float* w2, const float* w3, const float* a1,
                               const float* a2, const float* dy, int64_t lddy, float* dx, int64_t lddx, float* dw1, float* db1, float* dw2,
                               float* db2, float* dw3, float* db3, int64_t M, int64_t D, int64_t H1, int64_t H2, int64_t T, void* workspace,
                               size_t workspace_bytes, gt_stream_t stream_) {
  int rc = mh_check("gt_head_mlp_bwd", compute, M, D, H1, H2, T);
  if (rc) return rc;
  GT_CHECK_ARG(x && w1 && w2 && w3 && a1 && a2 && dy, "null buffer");
  GT_CHECK_ARG(dw1 && db1 && dw2 && db2 && dw3 && db3, "null gradient buffer");
  GT_CHECK_ARG(ldx >= D && lddy >= T && (!dx || lddx >= D), "a row pitch is shorter than its row");
  if (!workspace || workspace_bytes < gt_head_mlp_workspace_bytes(M, H1, H2)) {
    gt_set_error("gt_head_mlp_bwd: a workspace of %zu bytes is needed", gt_head_mlp_workspace_bytes(M, H1, H2));
    return GT_ERR_WORKSPACE;
  }
  hipStream_t stream = (hipStream_t)stream_;
  float* d1 = (float*)workspace;
  float* d2 = d1 + M * H1;
  MlpArgs a{};
  a.w1 = w1; a.w2 = w2; a.w3 = w3; a.a1c = a1; a.a2c = a2; a.dy = dy; a.a1 = d1; a.a2 = d2; a.y = dx;
  a.M = M; a.ldy = lddy; a.lddx = lddx; a.D = (int)D; a.H1 = (int)H1; a.H2 = (int)H2; a.T = (int)T;
  GtProfScope prof(GT_PROF_LINEAR, "head_mlp_bwd", stream_, {M, D, H1, H2, T});
  hipLaunchKernelGGL(k_mlp_bwd_rows, dim3((unsigned)gt_cdiv(M, MH_R)), dim3(256), 0, stream, a);
  MlpGradArgs g{};
  g.x = x; g.a1 = a1; g.a2 = a2; g.d1 = d1; g.d2 = d2; g.dy = dy;
  g.dw1 = dw1; g.db1 = db1; g.dw2 = dw2; g.db2 = db2; g.dw3 = dw3; g.db3 = db3;
  g.M = M; g.ldx = ldx; g.ldy = lddy; g.D = (int)D; g.H1 = (int)H1; g.H2 = (int)H2; g.T = (int)T;
  const int64_t elems = H1 * D + H1 + H2 * H1 + H2 + T * H2 + T;
  hipLaunchKernelGGL(k_mlp_bwd_params, dim3((unsigned)gt_cdiv(elems, 256)), dim3(256), 0, stream, g);
  GT_CHECK_LAUNCH();
  return GT_OK;
}
