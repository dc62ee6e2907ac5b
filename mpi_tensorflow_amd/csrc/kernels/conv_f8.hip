// OCP e4m3 (fp8) MFMA implicit-GEMM forward convolution for ResNet-18
// inference (docs/ACCURACY.md "ResNet-18 fp8 inference"), and the weight
// quantiser that feeds it.
//
// conv_bf16.hip's convs are bound by vector-L1 bytes per MFMA; here both
// operands are one byte an element, so a K tile of one tap x 64 channels is 64
// bytes a row of A (activations, fp8 NHWC) and of B (weights, fp8
// [tap][k][c], c contiguous, written by wq_f8):
//   * lowp_conv_core.h's geometry (256 threads, 2 x 2 waves, block tiles 128 x
//     64 and 64 x 64 by byte_conv_plan's rule, no split-K, no atomics), its A
//     loaders and its epilogue (F8Epi);
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
//     flight during this tile's MFMAs, one barrier a K tile (a small chunk
//     fills few CUs on layer 4; that is accepted).
// Two loaders (template flag HALO):
//   gather  R in {1, 3}, stride in {1, 2}: each K tile gathers its BM input
//           pixels of one tap (GatherA); K tiles tap-major;
//   halo    3x3 / stride 1 / pad 1: the halo image of a 64-channel chunk
//           (HaloA) is staged once, double-buffered, and the nine taps read
//           their A fragments from it; K tiles chunk-major.  conv3_kernel's
//           idea on byte rows.
#include <type_traits>

#include "lowp_conv_core.h"

namespace gops {
namespace cf8 {

using namespace lowp;

typedef int i32x8 __attribute__((ext_vector_type(8)));

// The operand tiles of K tile kt: load() issues the global loads into
// registers, store() writes them into the LDS buffers tile kt is read from.
// LDS: two A images of ASZ bytes, then two B tiles.
template <int BM, bool HALO>
struct Loader {
  using A = std::conditional_t<HALO, HaloA<BM>, GatherA<BM>>;
  static constexpr int ASZ = A::ASZ;
  static constexpr int BSZ = BN * PITCH;
  A a;
  const uint8_t* wb;  // this thread's 16 bytes of its B row at (tap 0, channel 0)
  size_t wtap;        // bytes of a tap of B
  int cpt, lo;        // chunks a tap; this thread's 16 bytes inside an LDS tile
  u32x4 rb;           // (not a uint4: copied memory to memory, that one lives in scratch)

  LOWP_DEV Loader(const ConvShape& s, const uint8_t* x, const uint8_t* wt, int m0, int n0)
      : a(s, x, m0) {
    const int lrow = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 16;
    wb = wt + (size_t)(n0 + lrow) * s.C + lc;
    wtap = (size_t)s.K * s.C, cpt = s.C / BK, lo = lrow * PITCH + lc;
  }
  LOWP_DEV void load(int kt) {
    int tap, ch;
    if constexpr (HALO) {
      ch = kt / 9, tap = kt - 9 * ch;
      if (tap == 0) a.load(ch);
    } else {
      tap = kt / cpt, ch = kt - tap * cpt;
      a.load(ch, tap);
    }
    rb = *reinterpret_cast<const u32x4*>(wb + tap * wtap + ch * BK);
  }
  LOWP_DEV void store(int kt, char* smem) const {
    if constexpr (HALO) {
      if (kt % 9 == 0) a.store(smem + ((kt / 9) & 1) * ASZ);
    } else {
      a.store(smem + (kt & 1) * ASZ);
    }
    *reinterpret_cast<u32x4*>(smem + 2 * ASZ + (kt & 1) * BSZ + lo) = rb;
  }
};

// one K tile of a 32 x 32 accumulator from the 32 bytes of this lane's A and B rows
template <int MF>
LOWP_DEV f32x16 mma_tile(const char* ap, const uint4 b0, const uint4 b1, f32x16 acc) {
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
LOWP_KERNEL(NT) void f8conv_kernel(const ConvShape s, const uint8_t* __restrict__ x,
                                   const uint8_t* __restrict__ wt, const F8Epi e,
                                   void* __restrict__ yv) {
  using LD = Loader<BM, HALO>;
  constexpr int TM = BM / 64;
  constexpr int ASZ = LD::ASZ, BSZ = LD::BSZ;
  __shared__ __attribute__((aligned(16))) char smem[2 * ASZ + 2 * BSZ];
  const Tile<BM> t(s);
  const int nk = s.R * s.S * (s.C / BK);
  LD ld(s, x, wt, t.m0, t.n0);
  // the epilogue's per-column and per-conv operands, loaded before the main
  // loop (fwd_kernel: a load behind the first stores would wait for them)
  const float fa = e.a2[t.co], fb = e.b[t.co];
  const float sres = e.res ? *e.s_res : 0.f;
  const float inv = OUT8 ? *e.inv_s_out : 1.f;
  int mask[TM];
  if constexpr (HALO) {
    zero_halo_rows(smem, ASZ, PITCH);
#pragma unroll
    for (int i = 0; i < TM; ++i) mask[i] = halo_mask(s, t.m0 + t.row(i), t.M);
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
    const char* bp = smem + 2 * ASZ + (kt & 1) * BSZ + (t.wn * 32 + t.r) * PITCH + 32 * t.h;
    const uint4 b0 = *reinterpret_cast<const uint4*>(bp);
    const uint4 b1 = *reinterpret_cast<const uint4*>(bp + 16);
    if constexpr (HALO) {
      const int chunk = kt / 9, tap = kt - 9 * chunk;
      const int shift = (tap / 3) * s.W + tap % 3;
      const char* A = smem + (chunk & 1) * ASZ + 32 * t.h;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = (mask[i] >> tap) & 1 ? t.row(i) + shift : HCAP;
        acc[i] = mma_tile<MF>(A + row * PITCH, b0, b1, acc[i]);
      }
    } else {
      const char* A = smem + (kt & 1) * ASZ + 32 * t.h;
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[i] = mma_tile<MF>(A + t.row(i) * PITCH, b0, b1, acc[i]);
    }
    if (more) ld.store(kt + 1, smem);
    block_sync();
  }
  f8_epilogue<BM, OUT8>(acc, e, fa, fb, sres, inv, t, (size_t)s.K, yv);
}

// scale(amax) = 2^j, j the least integer with 448 2^j >= amax; scale(0) = 1.
// Exact: amax = m 2^e with m in [0.5, 1) and 448 = 0.875 2^9, so j = e - 9 for
// m <= 0.875, else e - 8.  j is held to [-100, 100] so that the scale and its
// inverse are normal floats (docs/ACCURACY.md).
LOWP_DEV int scale_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int ex;
  const float m = frexpf(amax, &ex);
  const int j = m <= 0.875f ? ex - 9 : ex - 8;
  return min(max(j, -100), 100);
}

// Every conv's weights in ONE launch: jobs[j] = {w (HWIO fp32), out (fp8
// [tap][k][c]), taps, C, K, offset into sw, first block, 0} (int64), K / 32
// blocks a job, first blocks ascending.  A block owns 32 output channels:
// pass 1 takes max |w| over taps x C per channel (a max: no order dependence)
// and writes sw[k] = scale(amax); pass 2 re-reads the slice 32 x 32 at a time
// through an LDS transpose and writes the codes q(w / sw[k]), c contiguous.
LOWP_KERNEL(NT) void wq_f8_kernel(const long long* __restrict__ jobs, int njobs,
                                  float* __restrict__ sw) {
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
LOWP_KERNEL(NT) void f8_fold_kernel(const long long* __restrict__ jobs, int njobs,
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
  const dim3 grid = conv_grid(s, BM);
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

}  // namespace cf8

bool f8conv_ok(const ConvShape& s) {
  const long long M = (long long)s.N * s.OH * s.OW;
  return s.R == s.S && (s.R == 1 || s.R == 3) && (s.stride == 1 || s.stride == 2) && s.pad >= 0 &&
         s.pad < s.R && s.C >= 64 && s.C % 64 == 0 && s.K >= 64 && s.K % 64 == 0 && s.N >= 1 &&
         s.OH == (s.H + 2 * s.pad - s.R) / s.stride + 1 &&
         s.OW == (s.W + 2 * s.pad - s.R) / s.stride + 1 && s.OH >= 1 && s.OW >= 1 &&
         M + 128 < (1LL << 31) && (long long)s.N * s.H * s.W < (1LL << 31);
}

// (docs/PERF_NOTES.md holds the measurements behind g_form)
F8Plan f8conv_plan(const ConvShape& s, int form) {
  return lowp::byte_conv_plan(s, form, cf8::g_form, "f8conv");
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
