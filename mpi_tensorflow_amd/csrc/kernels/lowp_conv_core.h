// What the low-precision inference convs of ResNet-18 share (conv_f8.hip,
// conv_mx4.hip, conv_x3.hip; internal to those three files): the geometry of a
// block, the halo form's tap mask and zero row, the byte-row A loaders and the
// F8Epi epilogue of the two fp8-activation convs, and the host side's tile and
// form rule.  The K loops, the B operands and the quantisers are each file's
// own.
//
// Geometry: 256 threads, 2 x 2 waves; a block tile is BM x 64, BM in {64, 128},
// one 32 x 32 accumulator per 32 rows of a wave; fwd_kernel's XCD-aware block
// order; no split-K and no atomics, so one wave accumulates an output element
// over the K tiles in one fixed order.
// Halo form (3x3 / stride 1 / pad 1): the contiguous run of input pixels from
// one image row above the block's output pixels to one below (BM + 2 W + 2 <=
// HCAP rows) is staged once per channel chunk, double-buffered, and the nine
// taps read their A fragments from it at a per-lane shifted row; a tap outside
// the image (halo_mask) reads row HCAP, which is all zeros (zero_halo_rows).
#pragma once

#include <stdexcept>
#include <string>

#include "common.h"
#include "ops_generic.h"

namespace gops {
namespace lowp {

constexpr int BN = 64;
constexpr int NT = 256;
constexpr int HCAP = 248;  // halo rows an LDS image holds; row HCAP is all zeros
// byte rows (fp8 activations): a K tile row is 64 channels.  LDS rows are
// padded from 64 to 80 bytes (conv_f8.hip says why)
constexpr int BK = 64;
constexpr int PITCH = 80;

// 16 bytes of B on their way from global memory to LDS
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Built without the packed fp32 instructions (resnet_infer.hip says why).
#define LOWP_TARGET __attribute__((target("no-packed-fp32-ops")))
#define LOWP_DEV __device__ __forceinline__ LOWP_TARGET
// LOWP_KERNEL(NT) or LOWP_KERNEL(NT, waves a SIMD)
#define LOWP_KERNEL(...) __global__ __launch_bounds__(__VA_ARGS__) LOWP_TARGET

// (HIP's header helpers - make_uint4, __syncthreads, __uint_as_float - carry the
// default target features and would become real calls from these functions, so
// the few that are needed are written on builtins here)
LOWP_DEV uint4 zero4() {
  uint4 z;
  z.x = z.y = z.z = z.w = 0u;
  return z;
}
LOWP_DEV uint4 keep4(uint4 v, bool ok) {
  v.x = ok ? v.x : 0u, v.y = ok ? v.y : 0u, v.z = ok ? v.z : 0u, v.w = ok ? v.w : 0u;
  return v;
}
LOWP_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
LOWP_DEV float e4m3_to_f32(uint32_t byte) { return __builtin_amdgcn_cvt_f32_fp8((int)byte, 0); }
// q(v): clamp in fp32, then the hardware's round-to-nearest-even convert
LOWP_DEV uint32_t f32_to_e4m3(float v) {
  v = fminf(fmaxf(v, -448.f), 448.f);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xffu;
}
LOWP_DEV float pow2(int j) { return __builtin_bit_cast(float, (uint32_t)(j + 127) << 23); }

// This block's tile and this lane's place in it: lane (r, h) of wave (wm, wn)
// works on rows row(i) of the tile and holds output column co.
template <int BM>
struct Tile {
  int M, m0, n0, wm, wn, r, h, co;
  LOWP_DEV explicit Tile(const ConvShape& s) {
    M = s.N * s.OH * s.OW;
    const int mt = (M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    m0 = (bid % mt) * BM, n0 = (bid / mt) * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    wm = wave & 1, wn = wave >> 1, r = lane & 31, h = lane >> 5;
    co = n0 + wn * 32 + r;
  }
  // the tile row whose A fragment feeds accumulator i of this lane
  LOWP_DEV int row(int i) const { return wm * (BM / 2) + 32 * i + r; }
};

// halo: which of the nine taps of output row m lie inside the image
LOWP_DEV int halo_mask(const ConvShape& s, int m, int M) {
  const int px = m % s.W, py = (m / s.W) % s.H;
  int mask = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if (m < M && (unsigned)(py + t / 3 - 1) < (unsigned)s.H &&
        (unsigned)(px + t % 3 - 1) < (unsigned)s.W)
      mask |= 1 << t;
  return mask;
}

// halo: the zero row of both images (ASZ bytes each, rows of `row` bytes)
LOWP_DEV void zero_halo_rows(char* smem, int ASZ, int row) {
  const int tid = threadIdx.x, n16 = row / 16;
  if (tid < 2 * n16)
    *reinterpret_cast<uint4*>(smem + (tid / n16) * ASZ + HCAP * row + 16 * (tid % n16)) = zero4();
}

// The A operand of the byte-row convs.  load() issues the global loads into
// registers, store() writes them into an LDS image.  Every load is
// unconditional, from a pixel clamped into the tensor, and a pixel outside the
// image is zeroed in registers (no branch around a load).  Thread t owns bytes
// [16 (t & 3), +16) of rows (t >> 2) + 64 i.
//
// The halo image of one 64-channel chunk.
template <int BM>
struct HaloA {
  static constexpr int ASZ = (HCAP + 1) * PITCH;
  static constexpr int HLD = (HCAP + 63) / 64;  // 16-byte loads a thread
  const uint8_t* x;
  long long p0;  // the first pixel of the run
  int M, C, hr, lrow, lc;
  uint4 rh[HLD];
  LOWP_DEV HaloA(const ConvShape& s, const uint8_t* x_, int m0) : x(x_) {
    M = s.N * s.OH * s.OW, C = s.C, lrow = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 16;
    p0 = (long long)m0 - s.W - 1, hr = BM + 2 * s.W + 2;
  }
  LOWP_DEV void load(int ch) {
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const long long p = p0 + lrow + 64 * i, pc = p < 0 ? 0 : (p < M ? p : M - 1);
      rh[i] = keep4(*reinterpret_cast<const uint4*>(x + (size_t)pc * C + ch * BK + lc), p == pc);
    }
  }
  LOWP_DEV void store(char* A) const {
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const int j = lrow + 64 * i;
      if (j < hr) *reinterpret_cast<uint4*>(A + j * PITCH + lc) = rh[i];
    }
  }
};

// The gathered tile of one (chunk, tap): BM input pixels of the tap, R in {1,
// 3}, stride in {1, 2}.
template <int BM>
struct GatherA {
  static constexpr int ASZ = BM * PITCH;
  static constexpr int AR = BM / 64;
  const ConvShape s;
  int lrow, lc;
  const uint8_t* xb[AR];  // the input pixel of tap (0, 0) of this thread's AR rows
  int iy0[AR], ix0[AR];
  uint4 ra[AR];
  LOWP_DEV GatherA(const ConvShape& s_, const uint8_t* x, int m0) : s(s_) {
    const int M = s.N * s.OH * s.OW;
    lrow = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 16;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int m = m0 + lrow + 64 * i;
      if (m < M) {
        const int ox = m % s.OW, t = m / s.OW, oy = t % s.OH, n = t / s.OH;
        iy0[i] = oy * s.stride - s.pad, ix0[i] = ox * s.stride - s.pad;
        xb[i] = x + (size_t)n * s.H * s.W * s.C + lc;
      } else {  // a row past M: every tap is outside
        iy0[i] = -(1 << 20), ix0[i] = 0, xb[i] = x;
      }
    }
  }
  LOWP_DEV void load(int ch, int tap) {
    const int kh = tap / s.S, kw = tap - kh * s.S;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int iy = iy0[i] + kh, ix = ix0[i] + kw;
      const int yc = min(max(iy, 0), s.H - 1), xc = min(max(ix, 0), s.W - 1);
      ra[i] = keep4(*reinterpret_cast<const uint4*>(xb[i] + ((size_t)yc * s.W + xc) * s.C + ch * BK),
                    iy == yc && ix == xc);
    }
  }
  LOWP_DEV void store(char* A) const {
#pragma unroll
    for (int i = 0; i < AR; ++i)
      *reinterpret_cast<uint4*>(A + (lrow + 64 * i) * PITCH + lc) = ra[i];
  }
};

// F8Epi on the accumulators, fp32, in this order: v = fmaf(acc, a2[k], b[k]);
// v += s_res * float(res) (fp8, optional); ReLU; store q(v * inv_s_out) as fp8
// or bf16(v).  Lane (r, h) holds column co of rows mb + (q & 3) + 8 (q >> 2);
// the residual loads first (rows clamped into the tensor), the stores last.
// fa, fb, sres, inv: a2[co], b[co], *s_res, *inv_s_out, which the kernels load
// before the main loop (fwd_kernel: a load behind the first stores would wait
// for them).
template <int BM, bool OUT8>
LOWP_DEV void f8_epilogue(const f32x16 (&acc)[BM / 64], const F8Epi& e, float fa, float fb,
                          float sres, float inv, const Tile<BM>& t, size_t K, void* yv) {
  const uint8_t* res = reinterpret_cast<const uint8_t*>(e.res);
  const int M = t.M, co = t.co;
#pragma unroll
  for (int i = 0; i < BM / 64; ++i) {
    const int mb = t.m0 + t.wm * (BM / 2) + 32 * i + 4 * t.h;
    float rv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = min(mb + (q & 3) + 8 * (q >> 2), M - 1);
      rv[q] = res ? e4m3_to_f32(res[(size_t)m * K + co]) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = mb + (q & 3) + 8 * (q >> 2);
      float v = __builtin_fmaf(acc[i][q], fa, fb);
      if (res) v += sres * rv[q];
      if (e.relu) v = fmaxf(v, 0.f);
      if (m >= M) continue;
      if constexpr (OUT8)
        reinterpret_cast<uint8_t*>(yv)[(size_t)m * K + co] = (uint8_t)f32_to_e4m3(v * inv);
      else
        reinterpret_cast<__bf16*>(yv)[(size_t)m * K + co] = (__bf16)v;
    }
  }
}

// ---- host side

inline dim3 conv_grid(const ConvShape& s, int bm) {
  const int M = s.N * s.OH * s.OW;
  return dim3((unsigned)(((M + bm - 1) / bm) * (s.K / BN)));
}

inline bool halo_ok(const ConvShape& s, int bm) {
  return s.R == 3 && s.S == 3 && s.stride == 1 && s.pad == 1 && bm + 2 * s.W + 2 <= HCAP;
}

// The tile and form of a byte-row conv `name` (f8conv, mx4conv).  form 0 is the
// planner's choice: default_form where it applies.
inline F8Plan byte_conv_plan(const ConvShape& s, int form, int default_form, const char* name) {
  const std::string n(name);
  if (!f8conv_ok(s)) throw std::runtime_error(n + ": unsupported shape");
  if (form < 0 || form > 2)
    throw std::runtime_error(n + ": form must be 0, 1 (gather) or 2 (halo)");
  F8Plan p;
  const long long M = (long long)s.N * s.OH * s.OW;
  // 128-row tiles once they alone give every CU (256) a block
  p.bm = (M / 128) * (s.K / 64) >= 256 ? 128 : 64;
  p.form = form == 0 ? (default_form == 2 && halo_ok(s, p.bm) ? 2 : 1) : form;
  if (p.form == 2 && !halo_ok(s, p.bm))
    throw std::runtime_error(n + ": the halo form takes 3x3 / stride 1 / pad 1 with "
                                 "bm + 2 W + 2 <= 248");
  return p;
}

}  // namespace lowp
}  // namespace gops
