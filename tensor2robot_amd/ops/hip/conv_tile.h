// Shared tile core of the stride-1 NHWC bf16 MFMA convs (gfx950 / CDNA4):
// conv_s1.hip (staged + glds-ring kernels) and conv_s1_big.hip (c-chunk).
// Device-only.  Every kernel here maps one wave to 32 output pixels of a
// TH x TW tile (pixel p = wave*32 + m, row-major in the tile) and runs
// v_mfma_f32_32x32x16_bf16 with M = pixels, N = output channels.
//
// Fragment layouts (verified by the mfma_probe GPU test):
//   A row = l%32, k = (l>>5)*8+j;  B col = l%32 (same k map);
//   C/D col = l&31, row = (reg&3)+8*(reg>>2)+4*(l>>5).
// conv_mfma_step encodes the A/B maps (its callers only pick the A-row
// pixel p = wave*32 + l%32) and conv_scatter_acc is the only place that
// encodes the C/D map.

#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

typedef __hip_bfloat16 cbf16_t;
typedef __attribute__((ext_vector_type(8))) short cbf16x8;
typedef __attribute__((ext_vector_type(16))) float cf32x16;

// bf16 per n-row of the GLOBAL packed weight image [rs][c16][n][WPAD]
// (16 used + 8 pad; ops/conv.py pack_weights mirrors it).
#define WPAD 24

// Which tile this workgroup owns: image and top-left output pixel.
struct ConvTile {
  int img, oh0, ow0;
};

template <int TH, int TW>
__device__ __forceinline__ ConvTile conv_tile_decode(int tiles_h,
                                                     int tiles_w) {
  ConvTile t;
  long wg = blockIdx.x;
  t.img = wg / (tiles_h * tiles_w);
  const int trest = wg % (tiles_h * tiles_w);
  const int th = trest / tiles_w;
  const int tw = trest % tiles_w;
  t.oh0 = th * TH;
  t.ow0 = tw * TW;
  return t;
}

// Stage the halo_h x halo_w x C input halo of tile `t` into LDS in 16-B
// chunks, zero-filling out-of-image pixels.  HALO_PITCH: pixels per LDS
// halo row; XP: shorts per LDS pixel.
template <int C, int NTHREADS, int HALO_PITCH, int XP>
__device__ __forceinline__ void conv_stage_halo(
    const cbf16_t* __restrict__ x, short* xtile, const ConvTile& t,
    int halo_h, int halo_w, int pad, int H, int W) {
  constexpr int chunks = C >> 3;
  const int total = halo_h * halo_w * chunks;
  for (int i = threadIdx.x; i < total; i += NTHREADS) {
    const int chunk = i % chunks;
    const int pix = i / chunks;
    const int hrow = pix / halo_w, hcol = pix % halo_w;
    const int iy = t.oh0 - pad + hrow;
    const int ix = t.ow0 - pad + hcol;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
      v = *reinterpret_cast<const uint4*>(
          x + (((long)t.img * H + iy) * W + ix) * C + chunk * 8);
    }
    *reinterpret_cast<uint4*>(
        &xtile[(hrow * HALO_PITCH + hcol) * XP + chunk * 8]) = v;
  }
}

// One (r,s) tap: C16N x NT MFMAs.  `pix` is this lane's LDS halo pixel
// for the tap: lane l owns tile pixel p = wave*32 + l%32 (its A row), so
// pix = (p/TW + r)*HALO_PITCH + p%TW + s.  `xp`: shorts per LDS pixel.
// `w` points at the tap's weights laid out [c16][n][>=16]: `n_stride`
// shorts per n-row, `c16_rows` n-rows per c16 slab.
template <int C16N, int NT>
__device__ __forceinline__ void conv_mfma_step(
    cf32x16 (&acc)[NT], const short* xtile, int pix, int xp,
    const short* w, int n_stride, int c16_rows) {
  const int lane = threadIdx.x & 63;
  const int mrow = lane & 31;
  const int kgrp = lane >> 5;
#pragma unroll
  for (int c16 = 0; c16 < C16N; ++c16) {
    cbf16x8 a_frag = *reinterpret_cast<const cbf16x8*>(
        &xtile[pix * xp + c16 * 16 + kgrp * 8]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = nt * 32 + mrow;
      cbf16x8 b_frag = *reinterpret_cast<const cbf16x8*>(
          &w[(c16 * c16_rows + n) * n_stride + kgrp * 8]);
      acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
          a_frag, b_frag, acc[nt], 0, 0, 0);
    }
  }
}

// Epilogue: write the NT 32x32 accumulators of this wave to
// y[img][orow][ocol][n0 + nt*32 + col], skipping pixels past OH/OW.
template <int NT, int TW>
__device__ __forceinline__ void conv_scatter_acc(
    const cf32x16 (&acc)[NT], cbf16_t* __restrict__ y, const ConvTile& t,
    int OH, int OW, int K, int n0) {
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int ocol_n = lane & 31;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
      const int p = wave * 32 + m;
      const int orow = t.oh0 + p / TW;
      const int ocol = t.ow0 + p % TW;
      if (orow < OH && ocol < OW) {
        y[(((long)t.img * OH + orow) * OW + ocol) * K
          + n0 + nt * 32 + ocol_n] = __float2bfloat16(acc[nt][reg]);
      }
    }
  }
}
