// OCP e4m3 (fp8) MFMA implicit-GEMM forward convolution for ResNet-18
// inference (docs/ACCURACY.md "ResNet-18 fp8 inference"), and the weight
// quantiser that feeds it.
//
// conv_bf16.hip's convs are bound by vector-L1 bytes per MFMA; here both
// operands are one byte an element, so a K tile of one tap x 64 channels is 64
// bytes a row of A (activations, fp8 NHWC) and of B (weights, fp8
// [tap][k][c], c contiguous, written by wq_f8):
//   * 256 threads, 2 x 2 waves; block tiles 128 x 64 and 64 x 64 (f8conv_plan,
//     by M), one 32 x 32 accumulator per 32 rows of a wave;
//   * lane (r, h) of a wave reads bytes [32 h, 32 h + 32) of LDS row r of A and
//     of B (two ds_read_b128 each) - the SAME slot-to-k mapping for both
//     operands, and the two lane groups cover the 64-byte K tile once, so the
//     dot product does not depend on the hardware's k order inside a lane.
//     MF = 1: one v_mfma_scale_f32_32x32x64_f8f6f4 on the 32 bytes (both scale
//     operands 2^0); MF = 2: four v_mfma_f32_32x32x16_fp8_fp8 on 8 bytes each;
//   * LDS rows are padded from 64 to 80 bytes.  A ds_read_b128 is served 16
//     lanes a cycle over 64 banks x 4 B = 256 B; the 16 lanes are 16
//     consecutive rows at one h, so their 16-byte slots are (5 row + const)
//     mod 16 with an 80-byte pitch - 5 is odd, the 16 slots are distinct and
//     the read is conflict-free (a 64-byte pitch would put rows r and r + 4 on
//     the same banks: 4-way).  The ds_write_b128 of the loaders (4 rows x 4
//     slots a 16-lane group) collide 2-way on 3 of 16 lanes; reads outnumber
//     writes;
//   * 16-byte global loads, double-buffered LDS, the next tile's loads in
//     flight during this tile's MFMAs, one barrier a K tile, fwd_kernel's
//     XCD-aware block order;
//   * NO split-K and no atomics: one wave accumulates an output element over
//     the K tiles in one fixed order, so a row's result does not depend on the
//     rows that share its launch (a small chunk fills few CUs on layer 4; that
//     is accepted).
// Two loaders (template flag HALO):
//   gather  R in {1, 3}, stride in {1, 2}: each K tile gathers its BM input
//           pixels of one tap (zeros outside the image); K tiles tap-major;
//   halo    3x3 / stride 1 / pad 1: per 64-channel chunk the contiguous run of
//           input pixels from one image row above the block's output pixels to
//           one below (BM + 2 W + 2 rows of 64 bytes) is staged once, double-
//           buffered, and the nine taps read their A fragments from it at a
//           per-lane shifted row (taps outside the image read a zero row); K
//           tiles chunk-major.  conv3_kernel's idea on byte rows.
// The epilogue (F8Epi), fp32, in this order: v = fmaf(acc, a2[k], b[k]); v +=
// s_res * float(res) (fp8, optional); ReLU; store q(v * inv_s_out) as fp8 or
// bf16(v), q(v) = e4m3_rne(clamp(v, -448, 448)).
#include <stdexcept>

#include "common.h"
#include "ops_generic.h"

namespace gops {
namespace cf8 {

constexpr int BK = 64;     // bytes (channels) of a K tile row
constexpr int PITCH = 80;  // LDS row pitch, bytes
constexpr int BN = 64;
constexpr int NT = 256;
constexpr int HCAP = 248;  // halo rows an LDS image holds; row HCAP is all zeros
constexpr int HLD = (HCAP + 63) / 64;  // halo 16-byte loads a thread

typedef int i32x8 __attribute__((ext_vector_type(8)));

// Built without the packed fp32 instructions (resnet_infer.hip says why).
#define F8_TARGET __attribute__((target("no-packed-fp32-ops")))
#define F8_KERNEL __global__ __launch_bounds__(NT) F8_TARGET
#define F8_DEV __device__ __forceinline__ F8_TARGET

// (HIP's header helpers - make_uint4, __syncthreads, __uint_as_float - carry the
// default target features and would become real calls from these functions, so
// the few that are needed are written on builtins here)
F8_DEV uint4 zero4() {
  uint4 z;
  z.x = z.y = z.z = z.w = 0u;
  return z;
}
F8_DEV uint4 keep4(uint4 v, bool ok) {
  v.x = ok ? v.x : 0u, v.y = ok ? v.y : 0u, v.z = ok ? v.z : 0u, v.w = ok ? v.w : 0u;
  return v;
}
F8_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
F8_DEV float e4m3_to_f32(uint32_t byte) { return __builtin_amdgcn_cvt_f32_fp8((int)byte, 0); }
// q(v): clamp in fp32, then the hardware's round-to-nearest-even convert
F8_DEV uint32_t f32_to_e4m3(float v) {
  v = fminf(fmaxf(v, -448.f), 448.f);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xffu;
}

// The operand tiles of K tile kt: load() issues the global loads into
// registers, store() writes them into the LDS buffers tile kt is read from.
// Every load is unconditional, from a pixel clamped into the tensor, and a
// pixel outside the image is zeroed in registers (no branch around a load).
// LDS: two A images of ASZ bytes, then two B tiles.
template <int BM, bool HALO>
struct Loader {
  static constexpr int AR = BM / 64;
  static constexpr int ASZ = (HALO ? HCAP + 1 : BM) * PITCH;
  static constexpr int BSZ = BN * PITCH;
  const ConvShape s;
  const uint8_t* x;
  const uint8_t* wb;  // this thread's 16 bytes of B row lrow at (tap 0, channel 0)
  int M, cpt, lrow, lc;
  // gather: the input pixel of tap (0, 0) of this thread's AR rows
  const uint8_t* xb[AR];
  int iy0[AR], ix0[AR];
  uint4 ra[AR];
  // halo: the first pixel of the run, its rows
  long long p0;
  int hr;
  uint4 rh[HALO ? HLD : 1];
  uint4 rb;

  F8_DEV Loader(const ConvShape& s_, const uint8_t* x_, const uint8_t* wt, int m0, int n0)
      : s(s_), x(x_) {
    const int tid = threadIdx.x;
    M = s.N * s.OH * s.OW, cpt = s.C / BK, lrow = tid >> 2, lc = (tid & 3) * 16;
    wb = wt + (size_t)(n0 + lrow) * s.C + lc;
    if constexpr (HALO) {
      p0 = (long long)m0 - s.W - 1;
      hr = BM + 2 * s.W + 2;
    } else {
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
  }
  F8_DEV void load(int kt) {
    int tap, c0;
    if constexpr (HALO) {
      const int chunk = kt / 9;
      tap = kt - 9 * chunk, c0 = chunk * BK;
      if (tap == 0) {
#pragma unroll
        for (int i = 0; i < HLD; ++i) {
          const int j = lrow + 64 * i;
          const long long p = p0 + j, pc = p < 0 ? 0 : (p < M ? p : M - 1);
          rh[i] = keep4(*reinterpret_cast<const uint4*>(x + (size_t)pc * s.C + c0 + lc), p == pc);
        }
      }
    } else {
      tap = kt / cpt, c0 = (kt - tap * cpt) * BK;
      const int kh = tap / s.S, kw = tap - kh * s.S;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int iy = iy0[i] + kh, ix = ix0[i] + kw;
        const int yc = min(max(iy, 0), s.H - 1), xc = min(max(ix, 0), s.W - 1);
        ra[i] = keep4(*reinterpret_cast<const uint4*>(xb[i] + ((size_t)yc * s.W + xc) * s.C + c0),
                      iy == yc && ix == xc);
      }
    }
    rb = *reinterpret_cast<const uint4*>(wb + (size_t)tap * s.K * s.C + c0);
  }
  F8_DEV void store(int kt, char* smem) const {
    if constexpr (HALO) {
      const int chunk = kt / 9;
      if (kt - 9 * chunk == 0) {
        char* A = smem + (chunk & 1) * ASZ;
#pragma unroll
        for (int i = 0; i < HLD; ++i) {
          const int j = lrow + 64 * i;
          if (j < hr) *reinterpret_cast<uint4*>(A + j * PITCH + lc) = rh[i];
        }
      }
    } else {
      char* A = smem + (kt & 1) * ASZ;
#pragma unroll
      for (int i = 0; i < AR; ++i)
        *reinterpret_cast<uint4*>(A + (lrow + 64 * i) * PITCH + lc) = ra[i];
    }
    *reinterpret_cast<uint4*>(smem + 2 * ASZ + (kt & 1) * BSZ + lrow * PITCH + lc) = rb;
  }
};

// one K tile of a 32 x 32 accumulator from the 32 bytes of this lane's A and B rows
template <int MF>
F8_DEV f32x16 mma_tile(const char* ap, const uint4 b0, const uint4 b1, f32x16 acc) {
  const uint4 a0 = *reinterpret_cast<const uint4*>(ap);
  const uint4 a1 = *reinterpret_cast<const uint4*>(ap + 16);
  if constexpr (MF == 1) {
    const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w,
                      (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
    const i32x8 bv = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w,
                      (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
    // cbsz = blgp = 0: both operands e4m3; E8M0 scale 127 = 2^0 in every byte
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 0, 0, 0x7f7f7f7f, 0,
                                                           0x7f7f7f7f);
  } else {
    const uint32_t aw[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
    const uint32_t bw[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long a = (long)(((unsigned long)aw[2 * k + 1] << 32) | aw[2 * k]);
      const long b = (long)(((unsigned long)bw[2 * k + 1] << 32) | bw[2 * k]);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a, b, acc, 0, 0, 0);
    }
    return acc;
  }
}

template <int BM, int MF, bool OUT8, bool HALO>
F8_KERNEL void f8conv_kernel(const ConvShape s, const uint8_t* __restrict__ x,
                             const uint8_t* __restrict__ wt, const F8Epi e, void* __restrict__ yv) {
  using LD = Loader<BM, HALO>;
  constexpr int TM = BM / 64;
  constexpr int ASZ = LD::ASZ, BSZ = LD::BSZ;
  __shared__ __attribute__((aligned(16))) char smem[2 * ASZ + 2 * BSZ];
  const int M = s.N * s.OH * s.OW;
  const int mt = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid % mt) * BM, n0 = (bid / mt) * BN;
  const int nk = s.R * s.S * (s.C / BK);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  LD ld(s, x, wt, m0, n0);
  // the epilogue's per-column and per-conv operands, loaded before the main
  // loop (fwd_kernel: a load behind the first stores would wait for them)
  const int co = n0 + wn * 32 + r;
  const float fa = e.a2[co], fb = e.b[co];
  const float sres = e.res ? *e.s_res : 0.f;
  const float inv = OUT8 ? *e.inv_s_out : 1.f;
  // halo: which of the nine taps of this lane's rows lie inside the image
  int mask[TM];
  if constexpr (HALO) {
    if (tid < 2 * (PITCH / 16))  // the zero row of both images
      *reinterpret_cast<uint4*>(smem + (tid / (PITCH / 16)) * ASZ + HCAP * PITCH +
                                16 * (tid % (PITCH / 16))) = zero4();
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * (BM / 2) + 32 * i + r;
      const int px = m % s.W, py = (m / s.W) % s.H;
      mask[i] = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (m < M && (unsigned)(py + t / 3 - 1) < (unsigned)s.H &&
            (unsigned)(px + t % 3 - 1) < (unsigned)s.W)
          mask[i] |= 1 << t;
    }
  }
  f32x16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = zero16();
  ld.load(0);
  ld.store(0, smem);
  block_sync();
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) ld.load(kt + 1);
    const char* bp = smem + 2 * ASZ + (kt & 1) * BSZ + (wn * 32 + r) * PITCH + 32 * h;
    const uint4 b0 = *reinterpret_cast<const uint4*>(bp);
    const uint4 b1 = *reinterpret_cast<const uint4*>(bp + 16);
    if constexpr (HALO) {
      const int chunk = kt / 9, tap = kt - 9 * chunk;
      const int shift = (tap / 3) * s.W + tap % 3;
      const char* A = smem + (chunk & 1) * ASZ + 32 * h;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = (mask[i] >> tap) & 1 ? wm * (BM / 2) + 32 * i + r + shift : HCAP;
        acc[i] = mma_tile<MF>(A + row * PITCH, b0, b1, acc[i]);
      }
    } else {
      const char* A = smem + (kt & 1) * ASZ + 32 * h;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        acc[i] = mma_tile<MF>(A + (wm * (BM / 2) + 32 * i + r) * PITCH, b0, b1, acc[i]);
    }
    if (more) ld.store(kt + 1, smem);
    block_sync();
  }
  // lane (r, h) holds column co of rows mb + (q & 3) + 8 (q >> 2); the residual
  // loads first (rows clamped into the tensor), the stores last
  const uint8_t* res = reinterpret_cast<const uint8_t*>(e.res);
  const size_t K = s.K;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int mb = m0 + wm * (BM / 2) + 32 * i + 4 * h;
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

// scale(amax) = 2^j, j the least integer with 448 2^j >= amax; scale(0) = 1.
// Exact: amax = m 2^e with m in [0.5, 1) and 448 = 0.875 2^9, so j = e - 9 for
// m <= 0.875, else e - 8.  j is held to [-100, 100] so that the scale and its
// inverse are normal floats (docs/ACCURACY.md).
F8_DEV int scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int ex;
  const float m = frexpf(amax, &ex);
  const int j = m <= 0.875f ? ex - 9 : ex - 8;
  return min(max(j, -100), 100);
}
F8_DEV float pow2(int j) { return __builtin_bit_cast(float, (uint32_t)(j + 127) << 23); }

// Every conv's weights in ONE launch: jobs[j] = {w (HWIO fp32), out (fp8
// [tap][k][c]), taps, C, K, offset into sw, first block, 0} (int64), K / 32
// blocks a job, first blocks ascending.  A block owns 32 output channels:
// pass 1 takes max |w| over taps x C per channel (a max: no order dependence)
// and writes sw[k] = scale(amax); pass 2 re-reads the slice 32 x 32 at a time
// through an LDS transpose and writes the codes q(w / sw[k]), c contiguous.
F8_KERNEL void wq_f8_kernel(const long long* __restrict__ jobs, int njobs, float* __restrict__ sw) {
  __shared__ float t[32][33];
  __shared__ float red[8][32];
  __shared__ float inv_s[32];
  const int b = blockIdx.x;
  int j = 0;
  for (int i = 1; i < njobs; ++i)
    if (jobs[8 * i + 6] <= b) j = i;
  const long long* J = jobs + 8 * j;
  const float* w = reinterpret_cast<const float*>(J[0]);
  uint8_t* out = reinterpret_cast<uint8_t*>(J[1]);
  const int taps = (int)J[2], C = (int)J[3], K = (int)J[4], off = (int)J[5];
  const int k0 = (b - (int)J[6]) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  float am = 0.f;
  for (int row = ty; row < taps * C; row += 8) am = fmaxf(am, fabsf(w[(size_t)row * K + k0 + tx]));
  red[ty][tx] = am;
  block_sync();
  if (ty == 0) {
#pragma unroll
    for (int i = 1; i < 8; ++i) am = fmaxf(am, red[i][tx]);
    const int e = scale_exp(am);
    sw[off + k0 + tx] = pow2(e);
    inv_s[tx] = pow2(-e);
  }
  block_sync();
  for (int tap = 0; tap < taps; ++tap)
    for (int c0 = 0; c0 < C; c0 += 32) {
      const float* src = w + ((size_t)tap * C + c0) * K + k0;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[ty + 8 * i][tx] = src[(size_t)(ty + 8 * i) * K + tx];
      block_sync();
      uint8_t* dst = out + ((size_t)tap * K + k0) * C + c0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = ty + 8 * i;
        dst[(size_t)k * C + tx] = (uint8_t)f32_to_e4m3(t[tx][k] * inv_s[k]);
      }
      block_sync();
    }
}

// Per conv of the net, one block each: jobs[j] = {channel offset (into the
// bn_fold table, sw and a2), K, amax slot of the input, of the output, of the
// residual (-1: none), 0, 0, 0} (int64).  a2[k] = a[k] sw[k] s_in (the two
// scales are powers of two: exact), s_res and 1 / s_out into scal[j] and
// scal[njobs + j]; block 0 also writes 1 / s of amax slot 0 (the pool output)
// into scal[2 njobs].
F8_KERNEL void f8_fold_kernel(const long long* __restrict__ jobs, int njobs,
                              const float* __restrict__ fold, const float* __restrict__ sw,
                              const float* __restrict__ amax, float* __restrict__ a2,
                              float* __restrict__ scal) {
  const long long* J = jobs + 8 * blockIdx.x;
  const int off = (int)J[0], K = (int)J[1], in = (int)J[2], out = (int)J[3], rs = (int)J[4];
  const float s_in = pow2(scale_exp(amax[in]));
  for (int k = threadIdx.x; k < K; k += NT) a2[off + k] = fold[off + k] * sw[off + k] * s_in;
  if (threadIdx.x == 0) {
    scal[blockIdx.x] = rs >= 0 ? pow2(scale_exp(amax[rs])) : 0.f;
    scal[njobs + blockIdx.x] = pow2(-scale_exp(amax[out]));
    if (blockIdx.x == 0) scal[2 * njobs] = pow2(-scale_exp(amax[0]));
  }
}

template <int BM, int MF, bool HALO>
static void launch(const ConvShape& s, const void* x, const void* w, const F8Epi& e, void* y,
                   bool out_bf16, hipStream_t st) {
  const int M = s.N * s.OH * s.OW;
  const dim3 grid((unsigned)(((M + BM - 1) / BM) * (s.K / BN)));
  const uint8_t* x8 = reinterpret_cast<const uint8_t*>(x);
  const uint8_t* w8 = reinterpret_cast<const uint8_t*>(w);
  if (out_bf16)
    f8conv_kernel<BM, MF, false, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
  else
    f8conv_kernel<BM, MF, true, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
}

// The defaults are the measured choices (docs/PERF_NOTES.md "ResNet-18 fp8
// inference"): the 64-deep MFMA, and the halo loader wherever it applies.
static int g_mfma = 1;  // the MFMA form of mfma = 0 (f8conv_set_mfma)
static int g_form = 2;  // the loader of form = 0 where the halo loader applies (f8conv_set_form)

#undef F8_KERNEL
#undef F8_DEV
#undef F8_TARGET

}  // namespace cf8

static bool f8_halo_ok(const ConvShape& s, int bm) {
  return s.R == 3 && s.S == 3 && s.stride == 1 && s.pad == 1 && bm + 2 * s.W + 2 <= cf8::HCAP;
}

bool f8conv_ok(const ConvShape& s) {
  const long long M = (long long)s.N * s.OH * s.OW;
  return s.R == s.S && (s.R == 1 || s.R == 3) && (s.stride == 1 || s.stride == 2) && s.pad >= 0 &&
         s.pad < s.R && s.C >= 64 && s.C % 64 == 0 && s.K >= 64 && s.K % 64 == 0 && s.N >= 1 &&
         s.OH == (s.H + 2 * s.pad - s.R) / s.stride + 1 &&
         s.OW == (s.W + 2 * s.pad - s.R) / s.stride + 1 && s.OH >= 1 && s.OW >= 1 &&
         M + 128 < (1LL << 31) && (long long)s.N * s.H * s.W < (1LL << 31);
}

F8Plan f8conv_plan(const ConvShape& s, int form) {
  if (!f8conv_ok(s)) throw std::runtime_error("f8conv: unsupported shape");
  if (form < 0 || form > 2) throw std::runtime_error("f8conv: form must be 0, 1 (gather) or 2 (halo)");
  F8Plan p;
  const long long M = (long long)s.N * s.OH * s.OW;
  // 128-row tiles once they alone give every CU (256) a block
  p.bm = (M / 128) * (s.K / 64) >= 256 ? 128 : 64;
  // the planner's choice (docs/PERF_NOTES.md holds the measurements behind g_form)
  p.form = form == 0 ? (cf8::g_form == 2 && f8_halo_ok(s, p.bm) ? 2 : 1) : form;
  if (p.form == 2 && !f8_halo_ok(s, p.bm))
    throw std::runtime_error("f8conv: the halo form takes 3x3 / stride 1 / pad 1 with "
                             "bm + 2 W + 2 <= 248");
  return p;
}

void f8conv_set_mfma(int mf) {
  if (mf != 1 && mf != 2) throw std::runtime_error("f8conv: mfma must be 1 (32x32x64) or 2 (32x32x16)");
  cf8::g_mfma = mf;
}

void f8conv_set_form(int form) {
  if (form != 1 && form != 2) throw std::runtime_error("f8conv: the default form is 1 (gather) or 2 (halo)");
  cf8::g_form = form;
}

void f8conv(const ConvShape& s, const void* x, const void* w, const F8Epi& e, void* y,
            bool out_bf16, int form, int mfma, hipStream_t st) {
  const F8Plan p = f8conv_plan(s, form);
  if (!x || !w || !y || !e.a2 || !e.b || (e.res && !e.s_res) || (!out_bf16 && !e.inv_s_out))
    throw std::runtime_error("f8conv: null operand");
  if (mfma < 0 || mfma > 2) throw std::runtime_error("f8conv: mfma must be 0, 1 or 2");
  const int mf = mfma ? mfma : cf8::g_mfma;
  const bool halo = p.form == 2;
#define F8_GO(BM, MF)                                                       \
  (halo ? cf8::launch<BM, MF, true>(s, x, w, e, y, out_bf16, st)            \
        : cf8::launch<BM, MF, false>(s, x, w, e, y, out_bf16, st))
  if (p.bm == 128)
    mf == 1 ? F8_GO(128, 1) : F8_GO(128, 2);
  else
    mf == 1 ? F8_GO(64, 1) : F8_GO(64, 2);
#undef F8_GO
}

void wq_f8(const long long* jobs, int njobs, long long nblocks, float* sw, hipStream_t st) {
  if (njobs <= 0 || nblocks <= 0 || !jobs || !sw) throw std::runtime_error("wq_f8: bad job table");
  cf8::wq_f8_kernel<<<(unsigned)nblocks, cf8::NT, 0, st>>>(jobs, njobs, sw);
}

void f8_fold(const long long* jobs, int njobs, const float* fold, const float* sw,
             const float* amax, float* a2, float* scal, hipStream_t st) {
  if (njobs <= 0 || !jobs || !fold || !sw || !amax || !a2 || !scal)
    throw std::runtime_error("f8_fold: bad job table");
  cf8::f8_fold_kernel<<<njobs, cf8::NT, 0, st>>>(jobs, njobs, fold, sw, amax, a2, scal);
}

}  // namespace gops
