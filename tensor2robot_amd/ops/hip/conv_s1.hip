// Hand-written MFMA conv for stride-1 NHWC bf16 (gfx950 / CDNA4).
//
// Covers the Grasping44 stride-1 convs (5x5 SAME @79^2, 3x3 SAME/VALID,
// C=K=64) where MIOpen's igemm runs at ~15-20% MFMA utilization on
// these small-channel shapes (profiles/).  Backward-data is the same
// kernel on flipped/transposed prepacked weights.
//
// Design (cdna_hip_programming.md §3/§5, MI355X_MICROARCH.md):
//  * implicit GEMM: out[p, k] = sum_{r,s,c} x[p+D(r,s), c] * w[r,s,c,k],
//    v_mfma_f32_32x32x16_bf16; M = pixels, N = K, K' = C*R*S.  The tile
//    decode, halo staging, MFMA step and accumulator scatter (and the
//    fragment layouts they encode) live in conv_tile.h.
//  * every wave computes 32 pixels x all K channels of a TH x 16-pixel
//    tile.  The halo tile lives in LDS with a PADDED 144-B pixel stride
//    (linear 128-B stride = 16-way bank conflict on the A-fragment
//    ds_read_b128 -- the §5 GEMM trap).
//  * R*S <= 9 (staged kernel): 256 threads, 8x16 tile; ALL weight chunks
//    are staged ONCE ([rs][c16][n][16] image, 32-B n-stride = 2-way
//    conflict), so the main loop is barrier-free (C=K=64: ~106 KiB LDS).
//  * R*S > 9 (ring kernel, the 5x5): the weights do not fit, so one
//    (r,s) chunk at a time streams through an LDS ring via LDS-DMA.
//  * the grid is 1-D over (image, tile); K is never split.
//  * measured (same-box interleaved A/B vs MIOpen/CK):
//    3x3@27^2 3.4x, 3x3@14^2 3.7x; 5x5@79^2 -- see profiles/.
//  * all LDS in ONE __shared__ array (§5 trap 4a).

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "conv_tile.h"

#define TILE_H 8              // staged-kernel tile height
#define TILE_W 16
#define HALO_H (TILE_H + 4)   // supports R <= 5
#define HALO_W (TILE_W + 4)
#define XPITCH 72             // bf16 per pixel row in LDS (64 + 8 pad)

#define XTILE_BF16 (HALO_H * HALO_W * XPITCH)

// C16N: C/16.  NT_WG: 32-wide N tiles computed per workgroup.
// RS_CAP: compile-time R*S capacity of the staged weight image.
template <int C16N, int NT_WG, int RS_CAP>
__global__ void __launch_bounds__(256, 2)
conv_s1_nhwc_kernel(const cbf16_t* __restrict__ x,
                    const cbf16_t* __restrict__ wpk,
                    cbf16_t* __restrict__ y,
                    int N, int H, int W, int K,
                    int R, int S, int pad,
                    int OH, int OW, int tiles_h, int tiles_w) {
  constexpr int C = C16N * 16;
  constexpr int K_WG = NT_WG * 32;
  constexpr int WLDS = RS_CAP * C16N * K_WG * 16;
  __shared__ short lds[XTILE_BF16 + WLDS];
  short* xtile = lds;
  short* wall = lds + XTILE_BF16;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int n0 = blockIdx.y * K_WG;    // channel-group offset
  const ConvTile t = conv_tile_decode<TILE_H, TILE_W>(tiles_h, tiles_w);

  conv_stage_halo<C, 256, HALO_W, XPITCH>(
      x, xtile, t, TILE_H + R - 1, TILE_W + S - 1, pad, H, W);

  // ---- stage every weight chunk for this channel group ----
  // Global image: [rs][c16][n(K)][WPAD]; LDS image:
  // [rs][c16][n(K_WG)][16].  Two 16-B pieces per n-row.
  {
    const int rows = R * S * C16N * K_WG;
    for (int i = tid; i < rows * 2; i += 256) {
      const int nrow = i >> 1, half = (i & 1) * 8;
      const int nn = nrow % K_WG;
      const int rc = nrow / K_WG;          // rs * C16N + c16
      *reinterpret_cast<uint4*>(&wall[nrow * 16 + half]) =
          *reinterpret_cast<const uint4*>(
              &wpk[((long)rc * K + n0 + nn) * WPAD + half]);
    }
  }
  __syncthreads();

  // ---- barrier-free main loop ----
  cf32x16 acc[NT_WG];
#pragma unroll
  for (int nt = 0; nt < NT_WG; ++nt) acc[nt] = (cf32x16){};
  const int p = wave * 32 + (lane & 31);    // this lane's A-row pixel
  const int RS = R * S;
  for (int rs = 0; rs < RS; ++rs) {
    const int r = rs / S, s = rs % S;
    conv_mfma_step<C16N, NT_WG>(
        acc, xtile, (p / TILE_W + r) * HALO_W + (p % TILE_W + s), XPITCH,
        wall + rs * (C16N * K_WG * 16), 16, K_WG);
  }

  conv_scatter_acc<NT_WG, TILE_W>(acc, y, t, OH, OW, K, n0);
}

// ---------------------------------------------------------------------------
// glds-ring variant for the 5x5: weight chunks stream via LDS-DMA
// (global_load_lds) through a RING_DEPTH-slot ring with counted vmcnt +
// raw barriers (cdna_hip_programming.md §5 "glds, 2-3 LDS buffers" rows)
// — no register round-trip, no write pass, loads RING_DEPTH-1 chunks
// ahead.
// ---------------------------------------------------------------------------

__device__ __forceinline__ void conv_waitcnt_vm(int count) {
  // s_waitcnt imm: vmcnt[3:0], expcnt[6:4]=7, lgkmcnt[11:8]=15.
  // `count` = allowed outstanding glds pieces for this wave.
  switch (count) {
    case 0: __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8)); break;
    case 1: __builtin_amdgcn_s_waitcnt(1 | (7 << 4) | (15 << 8)); break;
    case 2: __builtin_amdgcn_s_waitcnt(2 | (7 << 4) | (15 << 8)); break;
    case 3: __builtin_amdgcn_s_waitcnt(3 | (7 << 4) | (15 << 8)); break;
    case 4: __builtin_amdgcn_s_waitcnt(4 | (7 << 4) | (15 << 8)); break;
    case 5: __builtin_amdgcn_s_waitcnt(5 | (7 << 4) | (15 << 8)); break;
    case 6: __builtin_amdgcn_s_waitcnt(6 | (7 << 4) | (15 << 8)); break;
    case 8: __builtin_amdgcn_s_waitcnt(8 | (7 << 4) | (15 << 8)); break;
    default:
      __builtin_amdgcn_s_waitcnt(10 | (7 << 4) | (15 << 8)); break;
  }
}

// WAVES=8: one 512-thread WG owns a 16x16 tile (1 WG/CU).  WAVES=4:
// a 256-thread WG owns an 8x16 tile -> 2 independent WGs/CU with
// uncoupled barriers, at the cost of streaming each weight chunk
// twice per 256 output pixels.
// No __launch_bounds__: the measured builds of this kernel never had an
// effective one (it sat behind an unbounded forward declaration), and
// adding it now changes the register allocation.
template <int C16N, int NTILES, int RING_DEPTH, int WAVES>
__global__ void
conv_s1_nhwc_ring_kernel(const cbf16_t* __restrict__ x,
                         const cbf16_t* __restrict__ wpk,
                         cbf16_t* __restrict__ y,
                         int N, int H, int W, int K,
                         int R, int S, int pad,
                         int OH, int OW, int tiles_h, int tiles_w) {
  constexpr int C = C16N * 16;
  constexpr int WBUF = C16N * NTILES * 32 * WPAD;      // bf16 per chunk
  constexpr int PIECES = (WBUF * 2 + 1023) / 1024;     // 1-KiB DMA pieces
  constexpr bool RAGGED = (WBUF * 2) % 1024 != 0;      // short last piece
  constexpr int NTHREADS = WAVES * 64;
  constexpr int TILE_HH = WAVES * 2;                   // tile = TH x 16
  constexpr int HALO_HH = TILE_HH + 4;
  __shared__ short lds[HALO_HH * HALO_W * XPITCH + RING_DEPTH * WBUF];
  short* xtile = lds;
  auto wbuf = [&](int slot) -> short* {
    return lds + HALO_HH * HALO_W * XPITCH + slot * WBUF;
  };

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const ConvTile t = conv_tile_decode<TILE_HH, TILE_W>(tiles_h, tiles_w);

  // Issuer wave w loads pieces [w*PPW, (w+1)*PPW) of each chunk and
  // counts its own vmcnt: WAVES=8 -> 6 issuer waves x 2 pieces at
  // PIECES=12; WAVES=4 -> 4 issuer waves x PIECES/4.  When PPW does not
  // divide PIECES, wave PIECES/PPW holds only the TAIL pieces.
  constexpr int ISSUERS = (WAVES == 8) ? 6 : WAVES;
  constexpr int PPW = (PIECES + ISSUERS - 1) / ISSUERS;
  constexpr int TAIL = PIECES % PPW;
  const bool issuer = wave < ISSUERS;
  const int my_pieces = (TAIL != 0 && wave == PIECES / PPW) ? TAIL : PPW;
  auto issue_chunk = [&](int rs, int slot) {
    if (!issuer) return;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int piece = wave * PPW + j;
      if (piece < PIECES &&
          (!RAGGED || piece * 512 + lane * 8 < WBUF)) {
        const cbf16_t* src = wpk + (long)rs * WBUF + piece * 512
                             + lane * 8;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) uint32_t*)src,
            (__attribute__((address_space(3))) uint32_t*)
                (wbuf(slot) + piece * 512),
            16, 0, 0);
      }
    }
  };

  conv_stage_halo<C, NTHREADS, HALO_W, XPITCH>(
      x, xtile, t, TILE_HH + R - 1, TILE_W + S - 1, pad, H, W);
  for (int cpre = 0; cpre < RING_DEPTH - 1 && cpre < R * S; ++cpre) {
    issue_chunk(cpre, cpre % RING_DEPTH);
  }
  // One full drain in the prologue (also covers the x-tile loads).
  __syncthreads();

  cf32x16 acc[NTILES];
#pragma unroll
  for (int nt = 0; nt < NTILES; ++nt) acc[nt] = (cf32x16){};
  const int p = wave * 32 + (lane & 31);    // this lane's A-row pixel
  const int RS = R * S;
  for (int rs = 0; rs < RS; ++rs) {
    const int r = rs / S, s = rs % S;
    const int slot = rs % RING_DEPTH;
    if (rs + RING_DEPTH - 1 < RS)
      issue_chunk(rs + RING_DEPTH - 1, (rs + RING_DEPTH - 1) % RING_DEPTH);
    if (issuer)
      conv_waitcnt_vm(min(RS - 1 - rs, RING_DEPTH - 1) * my_pieces);
    __builtin_amdgcn_s_barrier();     // chunk rs landed for everyone
    conv_mfma_step<C16N, NTILES>(
        acc, xtile, (p / TILE_W + r) * HALO_W + (p % TILE_W + s), XPITCH,
        wbuf(slot), WPAD, K);
    // Slot rs%RING_DEPTH is refilled by the DMA issued at iteration
    // rs+1 (chunk rs+RING_DEPTH): everyone must be done reading
    // before that DMA can be issued.
    __builtin_amdgcn_s_barrier();
  }

  conv_scatter_acc<NTILES, TILE_W>(acc, y, t, OH, OW, K, 0);
}

// ---------------------------------------------------------------------------
// Host wrapper
// ---------------------------------------------------------------------------

at::Tensor conv_s1_nhwc(at::Tensor x, at::Tensor wpk, int64_t K,
                        int64_t R, int64_t S, int64_t pad) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "conv_s1_nhwc: bf16 CUDA input required");
  TORCH_CHECK(x.dim() == 4 &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "conv_s1_nhwc: NCHW channels_last required");
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(C % 16 == 0 && C <= 64, "conv_s1_nhwc: C % 16, C <= 64");
  TORCH_CHECK(K % 32 == 0 && K <= 64, "conv_s1_nhwc: K % 32, K <= 64");
  TORCH_CHECK(R <= 5 && S <= 5, "conv_s1_nhwc: R,S <= 5");
  const int OH = H + 2 * pad - R + 1;
  const int OW = W + 2 * pad - S + 1;
  TORCH_CHECK(OH > 0 && OW > 0);
  auto y = at::empty({N, K, OH, OW},
                     x.options().memory_format(
                         at::MemoryFormat::ChannelsLast));
  auto stream = at::cuda::getCurrentCUDAStream();
  // One wave per 2 tile rows of 16 pixels: waves*2 x 16 tiles.
  auto launch = [&](auto kern, int waves) {
    const int tiles_h = (OH + waves * 2 - 1) / (waves * 2);
    const int tiles_w = (OW + TILE_W - 1) / TILE_W;
    const long grid = (long)N * tiles_h * tiles_w;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), 0,
                       stream.stream(),
                       (const cbf16_t*)x.data_ptr(),
                       (const cbf16_t*)wpk.data_ptr(),
                       (cbf16_t*)y.data_ptr(),
                       N, H, W, (int)K, (int)R, (int)S, (int)pad,
                       OH, OW, tiles_h, tiles_w);
  };
  const bool small = (R * S) <= 9;
  // Retired after losing (profiles/): 64x64 ring 6-deep 446 vs 477 TF,
  // 8-wave tile 478 vs 490-497 TF, s_setprio around the MFMAs -5%.
  if (small && C == 64 && K == 64)
    launch(conv_s1_nhwc_kernel<4, 2, 9>, 4);
  else if (small && C == 32 && K == 32)
    launch(conv_s1_nhwc_kernel<2, 1, 9>, 4);
  else if (small && C == 48 && K == 64)
    launch(conv_s1_nhwc_kernel<3, 2, 9>, 4);
  else if (small && C == 16 && K == 64)
    launch(conv_s1_nhwc_kernel<1, 2, 9>, 4);
  else if (small && C == 16 && K == 32)
    launch(conv_s1_nhwc_kernel<1, 1, 9>, 4);
  else if (!small && C == 64 && K == 64)
    launch(conv_s1_nhwc_ring_kernel<4, 2, 3, 4>, 4);
  else if (!small && C == 32 && K == 32)
    launch(conv_s1_nhwc_ring_kernel<2, 1, 6, 8>, 8);
  else if (!small && C == 48 && K == 64)
    launch(conv_s1_nhwc_ring_kernel<3, 2, 6, 8>, 8);
  else if (!small && C == 16 && K == 32)
    launch(conv_s1_nhwc_ring_kernel<1, 1, 6, 8>, 8);
  else
    TORCH_CHECK(false, "conv_s1_nhwc: unsupported C/K combo");
  return y;
}

// ---------------------------------------------------------------------------
// Single-kernel weight pack: [K,C,R,S] (torch, any float dtype widened to
// bf16 host-side = the .to(bf16) cast folds in here) -> the conv kernel's
// [rs][c16][n][WPAD] image.  transpose=true additionally swaps the C/K
// roles and flips r,s — the backward-data pack — so the python wrapper
// launches ONE kernel instead of ~7 tensor ops per conv per step.
// ---------------------------------------------------------------------------

// Element i of the packed image of w [K][C][R][S]: the source element,
// or zero in the pad columns.
__device__ __forceinline__ cbf16_t pack_conv_w_elem(
    const cbf16_t* __restrict__ w, long i, bool transpose,
    int K, int C, int R, int S) {
  // Output dims: C-role = transpose ? K : C; K-role = transpose ? C : K.
  const int crole = transpose ? K : C;
  const int krole = transpose ? C : K;
  const int cc = i % WPAD;
  long rest = i / WPAD;
  const int n = rest % krole;
  rest /= krole;
  const int c16 = rest % (crole / 16);
  const int rs = rest / (crole / 16);
  if (cc >= 16) return __float2bfloat16(0.0f);
  const int c = c16 * 16 + cc;
  int r = rs / S, s = rs % S;
  int kk, ci;
  if (transpose) {
    kk = c;          // original K index comes from the C-role dim
    ci = n;          // original C index comes from the K-role dim
    r = R - 1 - r;
    s = S - 1 - s;
  } else {
    kk = n;
    ci = c;
  }
  return w[(((long)kk * C + ci) * R + r) * S + s];
}

template <bool TRANSPOSE>
__global__ void __launch_bounds__(256)
pack_conv_w_kernel(const cbf16_t* __restrict__ w,   // [K][C][R][S]
                   cbf16_t* __restrict__ out,       // [rs][c16][n][WPAD]
                   int K, int C, int R, int S, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x)
    out[i] = pack_conv_w_elem(w, i, TRANSPOSE, K, C, R, S);
}

// One dispatch emitting BOTH the forward pack and the dgrad pack.
__global__ void __launch_bounds__(256)
pack_conv_w_pair_kernel(const cbf16_t* __restrict__ w,  // [K][C][R][S]
                        cbf16_t* __restrict__ outf,
                        cbf16_t* __restrict__ outb,
                        int K, int C, int R, int S,
                        long totalf, long totalb) {
  for (long ii = blockIdx.x * (long)blockDim.x + threadIdx.x;
       ii < totalf + totalb; ii += (long)gridDim.x * blockDim.x) {
    const bool tr = ii >= totalf;
    const long i = tr ? ii - totalf : ii;
    (tr ? outb : outf)[i] = pack_conv_w_elem(w, i, tr, K, C, R, S);
  }
}

// Host side of both packs: w as contiguous bf16, the empty packed image
// of each requested direction ([0] forward, [1] transposed) and the grid
// covering their elements.
struct PackPlan {
  at::Tensor w, out[2];
  long total[2] = {0, 0};
  int K, C, R, S, grid;
};

static PackPlan pack_plan(at::Tensor w, bool fwd, bool bwd) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 4, "pack_conv_w: 4D CUDA");
  PackPlan p;
  p.w = w.contiguous();
  if (p.w.scalar_type() != at::kBFloat16) p.w = p.w.to(at::kBFloat16);
  p.K = w.size(0), p.C = w.size(1), p.R = w.size(2), p.S = w.size(3);
  for (int tr = 0; tr < 2; ++tr) {
    if (!(tr ? bwd : fwd)) continue;
    const int crole = tr ? p.K : p.C;
    const int krole = tr ? p.C : p.K;
    TORCH_CHECK(crole % 16 == 0, "pack_conv_w: C-role % 16");
    p.out[tr] = at::empty({(long)p.R * p.S, crole / 16, krole, WPAD},
                          p.w.options());
    p.total[tr] = p.out[tr].numel();
  }
  p.grid = (int)std::min<long>((p.total[0] + p.total[1] + 255) / 256,
                               4096);
  return p;
}

at::Tensor pack_conv_w(at::Tensor w, bool transpose) {
  PackPlan p = pack_plan(w, !transpose, transpose);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kern = transpose ? pack_conv_w_kernel<true>
                        : pack_conv_w_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), 0, stream.stream(),
                     (const cbf16_t*)p.w.data_ptr(),
                     (cbf16_t*)p.out[transpose].data_ptr(),
                     p.K, p.C, p.R, p.S, p.total[transpose]);
  return p.out[transpose];
}

std::vector<at::Tensor> pack_conv_w_pair(at::Tensor w) {
  // Halves the per-step pack launches and takes the dgrad pack off the
  // backward critical path.
  PackPlan p = pack_plan(w, true, true);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(pack_conv_w_pair_kernel, dim3(p.grid), dim3(256), 0,
                     stream.stream(), (const cbf16_t*)p.w.data_ptr(),
                     (cbf16_t*)p.out[0].data_ptr(),
                     (cbf16_t*)p.out[1].data_ptr(),
                     p.K, p.C, p.R, p.S, p.total[0], p.total[1]);
  return {p.out[0], p.out[1]};
}

// ---------------------------------------------------------------------------
// Fused space-to-depth for the 6x6/2 stem: [N][H][W][3] bf16 (NHWC) ->
// [N][H/2][W/2][16] with c' = dr*6 + ds*3 + c and slots 12..15 zero.
// One global read + one write replaces the torch zeros/permute/copy
// chain (4 kernels, ~3x the bytes).  The 6 taps of each (dr) row are
// contiguous in NHWC (x[n, 2oy+dr, 2ox..2ox+1, 0..2]) and every
// offset is u32-aligned (element offsets are multiples of 6), so the
// read is 2x3 dwords and the write is 2 dwordx4 per output pixel.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) unsigned int cuint4v;

__global__ void __launch_bounds__(256)
s2d_stem_kernel(const unsigned int* __restrict__ x,
                cuint4v* __restrict__ y,
                long total, int H, int W, int OH, int OW) {
  const int row_u32 = (W * 3) >> 1;   // u32 per input row (W even)
  for (long p = blockIdx.x * 256L + threadIdx.x; p < total;
       p += (long)gridDim.x * 256) {
    const int ox = (int)(p % OW);
    long rest = p / OW;
    const int oy = (int)(rest % OH);
    const long n = rest / OH;
    const long base = (((n * H + 2L * oy) * W) * 3 >> 1) + 3L * ox;
    const unsigned int a0 = x[base], a1 = x[base + 1], a2 = x[base + 2];
    const long b = base + row_u32;
    const unsigned int b0 = x[b], b1 = x[b + 1], b2 = x[b + 2];
    y[p * 2] = cuint4v{a0, a1, a2, b0};
    y[p * 2 + 1] = cuint4v{b1, b2, 0u, 0u};
  }
}

at::Tensor s2d_stem(at::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16,
              "s2d_stem: bf16 CUDA input required");
  TORCH_CHECK(x.dim() == 4 && x.size(1) == 3 &&
              x.is_contiguous(at::MemoryFormat::ChannelsLast),
              "s2d_stem: [N,3,H,W] channels_last required");
  const int N = x.size(0), H = x.size(2), W = x.size(3);
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "s2d_stem: even H, W required");
  const int OH = H / 2, OW = W / 2;
  auto y = at::empty({N, 16, OH, OW},
                     x.options().memory_format(
                         at::MemoryFormat::ChannelsLast));
  const long total = (long)N * OH * OW;
  const long blocks = std::min((total + 255) / 256, 8192L);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(s2d_stem_kernel, dim3(blocks), dim3(256), 0,
                     stream.stream(),
                     (const unsigned int*)x.data_ptr(),
                     (cuint4v*)y.data_ptr(), total, H, W, OH, OW);
  return y;
}