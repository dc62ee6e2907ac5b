// OCP microscaling FP4 (MXFP4) weights x e4m3 activations: the MFMA implicit-
// GEMM forward convolution of ResNet-18 --dtype mxfp4 inference
// (docs/ACCURACY.md "ResNet-18 mxfp4 inference"), and the weight quantiser that
// feeds it.
//
// conv_f8.hip's geometry (256 threads, 2 x 2 waves, block tiles 128 x 64 and
// 64 x 64 by f8conv's rule, one 32 x 32 accumulator per 32 rows of a wave, no
// split-K, no atomics, one fixed accumulation order, XCD-aware block order) and
// its epilogue (F8Epi); the B operand and the K loop are this file's own.
//
// MFMA.  One v_mfma_scale_f32_32x32x64_f8f6f4 per 32 x 32 tile per (tap,
// 64-channel chunk): cbsz = 0, A is e4m3, block scale 2^0; blgp = 4, B is
// e2m1, 16 bytes in the low four dwords, element i of the lane in bits [4 i,
// 4 i + 4), and its block scale is the lane's own E8M0 byte (opsel 0).  The two
// formats index k differently inside a lane (measured on the MI355X with an
// identity activation): of lane (r, h), the 4-bit operand's element i is k =
// 32 h + i, but the 8-bit operand's dwords 0-3 are k = 16 h + [0, 16) and its
// dwords 4-7 k = 32 + 16 h + [0, 16).  So a lane reads bytes [16 h, 16 h + 16)
// and [32 + 16 h, 48 + 16 h) of LDS row r of A (two ds_read_b128), and holds
// exactly one MX block of B: the 32 channels [32 h, 32 h + 32) of output
// channel r of one tap.  One byte a lane is the whole scale traffic, and the
// per-output-channel weight scale of the fp8 path drops out of the epilogue.
//
// Weight slabs (written by wq_mx4, read here).  One contiguous slab per (64-
// wide output-channel tile nt, 64-channel chunk ch), slab nt * (C / 64) + ch of
// a conv, taps * 2176 bytes each:
//   codes   for each tap, each 32-column group g, each h, each r: the 16 bytes
//           of lane (r, h) - channels 64 ch + 32 h + [0, 32) of output channel
//           64 nt + 32 g + r, the even channel in the low nibble; byte offset
//           (((tap * 2 + g) * 2 + h) * 32 + r) * 16;
//   scales  behind the codes (offset taps * 2048), one E8M0 byte a block, in
//           the same (tap, g, h, r) order.
// A slab is staged by a linear 16-byte copy.  A wave's ds_read_b128 of B hits
// 1024 contiguous bytes (16 bytes a lane, lane order), so it needs no padding
// and has no bank conflicts; its scale read is 64 contiguous bytes.
//
// K loop, chunk-major in both forms (template flag HALO):
//   halo    3x3 / stride 1 / pad 1 (f8conv's condition): A is f8conv's halo
//           image (pitch 80, a zero row, per-lane tap masks), double-buffered;
//           the 9-tap slab (19,584 bytes) is single-buffered.  Per chunk the
//           next chunk's halo and slab loads are issued into registers, the
//           nine taps run back to back from LDS with no barrier between them,
//           then the halo registers go to the other image, a barrier, the slab
//           registers over the slab, a barrier: two barriers a chunk where
//           f8conv takes nine.  LDS 39,840 + 19,584 bytes (static).
//   gather  R in {1, 3}, stride in {1, 2}: f8conv's per-tap gathered A tile,
//           double-buffered, one barrier a tap; A tiles are small here, so the
//           slab is double-buffered too (20,480 + 39,168 bytes at BM = 128) and
//           a 1x1 conv keeps one barrier a K tile.
#include <stdexcept>

#include "common.h"
#include "ops_generic.h"

namespace gops {
namespace cmx4 {

constexpr int BK = 64;     // channels (bytes of A) of a K tile row
constexpr int PITCH = 80;  // LDS row pitch of A, bytes (conv_f8.hip says why)
constexpr int BN = 64;
constexpr int NT = 256;
constexpr int HCAP = 248;  // halo rows an LDS image holds; row HCAP is all zeros
constexpr int HLD = (HCAP + 63) / 64;  // halo 16-byte loads a thread
constexpr int TAPB = 2048 + 128;       // slab bytes a tap: codes, scales
constexpr int SLAB9 = 9 * TAPB;
constexpr int SLD = (SLAB9 / 16 + NT - 1) / NT;  // slab 16-byte loads a thread

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Built without the packed fp32 instructions (resnet_infer.hip says why).
#define MX_TARGET __attribute__((target("no-packed-fp32-ops")))
// (two waves a SIMD: the two blocks a CU's LDS holds)
#define MX_KERNEL __global__ __launch_bounds__(NT, 2) MX_TARGET
#define MX_DEV __device__ __forceinline__ MX_TARGET

// (as in conv_f8.hip: HIP's header helpers carry the default target features,
// so the few that are needed are written on builtins)
MX_DEV uint4 zero4() {
  uint4 z;
  z.x = z.y = z.z = z.w = 0u;
  return z;
}
MX_DEV uint4 keep4(uint4 v, bool ok) {
  v.x = ok ? v.x : 0u, v.y = ok ? v.y : 0u, v.z = ok ? v.z : 0u, v.w = ok ? v.w : 0u;
  return v;
}
MX_DEV void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
MX_DEV float e4m3_to_f32(uint32_t byte) { return __builtin_amdgcn_cvt_f32_fp8((int)byte, 0); }
MX_DEV uint32_t f32_to_e4m3(float v) {
  v = fminf(fmaxf(v, -448.f), 448.f);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.f, 0, false) & 0xffu;
}

// The slab of one chunk: load() issues this thread's 16-byte global loads,
// store() writes them to an LDS slab.  n16 = taps * 136 vectors.
struct Slab {
  u32x4 rs[SLD];
  MX_DEV void load(const uint8_t* g, int n16) {
#pragma unroll
    for (int i = 0; i < SLD; ++i) {
      const int j = threadIdx.x + NT * i;
      rs[i] = reinterpret_cast<const u32x4*>(g)[j < n16 ? j : 0];
    }
  }
  MX_DEV void store(char* lds, int n16) const {
#pragma unroll
    for (int i = 0; i < SLD; ++i) {
      const int j = threadIdx.x + NT * i;
      if (j < n16) reinterpret_cast<u32x4*>(lds)[j] = rs[i];
    }
  }
};

// f8conv's halo image of one 64-channel chunk: the run of input pixels from one
// image row above the block's output pixels to one below, clamped into the
// tensor, zeros outside it.  load() issues the global loads into registers,
// store() writes them into image ch & 1.
template <int BM>
struct HaloA {
  const uint8_t* x;
  long long p0;
  int M, C, hr, lrow, lc;
  uint4 rh[HLD];
  MX_DEV HaloA(const ConvShape& s, const uint8_t* x_, int m0) : x(x_) {
    M = s.N * s.OH * s.OW, C = s.C, lrow = threadIdx.x >> 2, lc = (threadIdx.x & 3) * 16;
    p0 = (long long)m0 - s.W - 1, hr = BM + 2 * s.W + 2;
  }
  MX_DEV void load(int ch) {
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const long long p = p0 + lrow + 64 * i, pc = p < 0 ? 0 : (p < M ? p : M - 1);
      rh[i] = keep4(*reinterpret_cast<const uint4*>(x + (size_t)pc * C + ch * BK + lc), p == pc);
    }
  }
  MX_DEV void store(char* A) const {
#pragma unroll
    for (int i = 0; i < HLD; ++i) {
      const int j = lrow + 64 * i;
      if (j < hr) *reinterpret_cast<uint4*>(A + j * PITCH + lc) = rh[i];
    }
  }
};

// f8conv's gathered A tile of one (chunk, tap): BM input pixels of the tap.
// Every load is unconditional, from a pixel clamped into the tensor, and a
// pixel outside the image is zeroed in registers.
template <int BM>
struct GatherA {
  static constexpr int AR = BM / 64;
  const ConvShape s;
  int lrow, lc;
  const uint8_t* xb[AR];  // the input pixel of tap (0, 0) of this thread's AR rows
  int iy0[AR], ix0[AR];
  uint4 ra[AR];
  MX_DEV GatherA(const ConvShape& s_, const uint8_t* x, int m0) : s(s_) {
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
  MX_DEV void load(int ch, int tap) {
    const int kh = tap / s.S, kw = tap - kh * s.S;
#pragma unroll
    for (int i = 0; i < AR; ++i) {
      const int iy = iy0[i] + kh, ix = ix0[i] + kw;
      const int yc = min(max(iy, 0), s.H - 1), xc = min(max(ix, 0), s.W - 1);
      ra[i] = keep4(*reinterpret_cast<const uint4*>(xb[i] + ((size_t)yc * s.W + xc) * s.C + ch * BK),
                    iy == yc && ix == xc);
    }
  }
  MX_DEV void store(char* A) const {
#pragma unroll
    for (int i = 0; i < AR; ++i)
      *reinterpret_cast<uint4*>(A + (lrow + 64 * i) * PITCH + lc) = ra[i];
  }
};

// one (tap, chunk) of a 32 x 32 accumulator: the lane's two 16-byte runs of A
// (ap = its row + 16 h), its 16 bytes of B codes and its block scale
MX_DEV f32x16 mma_tile(const char* ap, const uint4 b, int scale, f32x16 acc) {
  const uint4 a0 = *reinterpret_cast<const uint4*>(ap);
  const uint4 a1 = *reinterpret_cast<const uint4*>(ap + 32);
  const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w,
                    (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const i32x8 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  // cbsz 0: A e4m3, scale 2^0; blgp 4: B e2m1, scale byte 0 of `scale`
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 4, 0, 0x7f7f7f7f, 0, scale);
}

// F8Epi on the accumulators: lane (r, h) holds column co of rows mb + (q & 3)
// + 8 (q >> 2); the residual loads first (rows clamped into the tensor), the
// stores last
template <int TM, bool OUT8>
MX_DEV void epilogue(const f32x16 (&acc)[TM], const F8Epi& e, float fa, float fb, float sres,
                     float inv, int mrow, int M, int co, size_t K, void* yv) {
  const uint8_t* res = reinterpret_cast<const uint8_t*>(e.res);
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int mb = mrow + 32 * i;
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

template <int BM, bool OUT8, bool HALO>
MX_KERNEL void mx4conv_kernel(const ConvShape s, const uint8_t* __restrict__ x,
                              const uint8_t* __restrict__ wt, const F8Epi e, void* __restrict__ yv) {
  constexpr int TM = BM / 64;
  constexpr int ASZ = (HALO ? HCAP + 1 : BM) * PITCH;
  __shared__ __attribute__((aligned(16))) char smem[2 * ASZ + (HALO ? 1 : 2) * SLAB9];
  char* const sl = smem + 2 * ASZ;
  const int M = s.N * s.OH * s.OW;
  const int mt = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid % mt) * BM, n0 = (bid / mt) * BN;
  const int taps = s.R * s.S, nch = s.C / BK;
  const int n16 = taps * (TAPB / 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  // this block's slabs: chunk ch at ws + ch * taps * TAPB
  const uint8_t* ws = wt + (size_t)(n0 / BN) * nch * taps * TAPB;
  // this lane's B codes and scale byte of tap 0 inside a slab
  const int bo = wn * 1024 + lane * 16, so = taps * 2048 + wn * 64 + lane;
  const int co = n0 + wn * 32 + r;
  const float fa = e.a2[co], fb = e.b[co];
  const float sres = e.res ? *e.s_res : 0.f;
  const float inv = OUT8 ? *e.inv_s_out : 1.f;
  f32x16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = zero16();
  Slab sb;
  if constexpr (HALO) {
    if (tid < 2 * (PITCH / 16))  // the zero row of both images
      *reinterpret_cast<uint4*>(smem + (tid / (PITCH / 16)) * ASZ + HCAP * PITCH +
                                16 * (tid % (PITCH / 16))) = zero4();
    // which of the nine taps of this lane's rows lie inside the image
    int mask[TM];
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
    HaloA<BM> ha(s, x, m0);
    ha.load(0);
    sb.load(ws, n16);
    ha.store(smem);
    sb.store(sl, n16);
    block_sync();
    for (int ch = 0; ch < nch; ++ch) {
      const bool more = ch + 1 < nch;
      if (more) {
        ha.load(ch + 1);
        sb.load(ws + (size_t)(ch + 1) * SLAB9, n16);
      }
      const char* A = smem + (ch & 1) * ASZ + 16 * h;
      // (a filter row at a time: unrolled over all nine taps the fragment
      // loads are hoisted together and spill)
#pragma unroll 1
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int tap = 3 * kh + kw;
          const uint4 b = *reinterpret_cast<const uint4*>(sl + tap * 2048 + bo);
          const int sc = *reinterpret_cast<const uint8_t*>(sl + tap * 128 + so);
          const int shift = kh * s.W + kw;
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const int row = (mask[i] >> tap) & 1 ? wm * (BM / 2) + 32 * i + r + shift : HCAP;
            acc[i] = mma_tile(A + row * PITCH, b, sc, acc[i]);
          }
        }
      if (more) {
        // the other image: its readers passed the barrier that ended chunk ch - 1
        ha.store(smem + ((ch + 1) & 1) * ASZ);
        block_sync();  // every wave has read this chunk's slab
        sb.store(sl, n16);
        block_sync();
      }
    }
  } else {
    GatherA<BM> ga(s, x, m0);
    const size_t slab = (size_t)taps * TAPB;
    ga.load(0, 0);
    sb.load(ws, n16);
    ga.store(smem);
    sb.store(sl, n16);
    block_sync();
    int kt = 0;
    for (int ch = 0; ch < nch; ++ch) {
      const char* S0 = sl + (ch & 1) * SLAB9;
      for (int tap = 0; tap < taps; ++tap, ++kt) {
        const bool last = tap + 1 == taps, more = !last || ch + 1 < nch;
        if (more) ga.load(last ? ch + 1 : ch, last ? 0 : tap + 1);
        if (last && more) sb.load(ws + (size_t)(ch + 1) * slab, n16);
        const uint4 b = *reinterpret_cast<const uint4*>(S0 + tap * 2048 + bo);
        const int sc = *reinterpret_cast<const uint8_t*>(S0 + tap * 128 + so);
        const char* A = smem + (kt & 1) * ASZ + 16 * h;
#pragma unroll
        for (int i = 0; i < TM; ++i)
          acc[i] = mma_tile(A + (wm * (BM / 2) + 32 * i + r) * PITCH, b, sc, acc[i]);
        if (more) ga.store(smem + ((kt + 1) & 1) * ASZ);
        // the other slab: its readers passed the barrier that ended chunk ch - 1
        if (last && more) sb.store(sl + ((ch + 1) & 1) * SLAB9, n16);
        block_sync();
      }
    }
  }
  epilogue<TM, OUT8>(acc, e, fa, fb, sres, inv, m0 + wm * (BM / 2) + 4 * h, M, co, (size_t)s.K, yv);
}

MX_DEV float pow2(int j) { return __builtin_bit_cast(float, (uint32_t)(j + 127) << 23); }

// E of a block: the least integer with 6 2^E >= amax, 0 for an all-zero block,
// held to [-100, 100].  Exact: amax = m 2^e with m in [0.5, 1) and 6 = 0.75
// 2^3, so E = e - 3 for m <= 0.75, else e - 2.
MX_DEV int block_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int ex;
  const float m = frexpf(amax, &ex);
  return min(max(m <= 0.75f ? ex - 3 : ex - 2, -100), 100);
}

// e2m1 code of v = w 2^-E (exact): the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6},
// a tie to the even 3-bit magnitude index; w's sign in bit 3
MX_DEV uint32_t e2m1(float w, float inv) {
  const float a = fabsf(w) * inv;
  const uint32_t idx = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                       (a >= 3.5f) + (a > 5.f);
  return idx | (w < 0.f ? 8u : 0u);
}

// Every conv's weights in ONE launch: jobs[j] = {w (HWIO fp32), out (slabs),
// taps, C, K, 0, first block, 0} (int64), (K / 64) (C / 64) blocks a job -
// one a slab - first blocks ascending.  A thread owns one MX block at a time:
// (tap, h, k) = the 32 channels 64 ch + 32 h + [0, 32) of output channel k of
// the tile; the 64 threads of a wave read 64 consecutive k (256 bytes a
// channel).  The block's amax is a max over its 32 values: no order dependence.
MX_KERNEL void wq_mx4_kernel(const long long* __restrict__ jobs, int njobs) {
  const int b = blockIdx.x;
  int j = 0;
  for (int i = 1; i < njobs; ++i)
    if (jobs[8 * i + 6] <= b) j = i;
  const long long* J = jobs + 8 * j;
  const float* w = reinterpret_cast<const float*>(J[0]);
  const int taps = (int)J[2], C = (int)J[3], K = (int)J[4];
  const int local = b - (int)J[6], nch = C / BK;
  const int nt = local / nch, ch = local - nt * nch;
  uint8_t* slab = reinterpret_cast<uint8_t*>(J[1]) + (size_t)local * taps * TAPB;
  const int k = threadIdx.x & 63, h = (threadIdx.x >> 6) & 1;
  for (int tap = threadIdx.x >> 7; tap < taps; tap += 2) {
    const float* src = w + ((size_t)tap * C + ch * BK + 32 * h) * K + nt * BN + k;
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      v[i] = src[(size_t)i * K];
      am = fmaxf(am, fabsf(v[i]));
    }
    const int E = block_exp(am);
    const float inv = pow2(-E);
    uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 32; ++i) pk[i >> 3] |= e2m1(v[i], inv) << (4 * (i & 7));
    const int slot = ((tap * 2 + (k >> 5)) * 2 + h) * 32 + (k & 31);
    uint4 o;
    o.x = pk[0], o.y = pk[1], o.z = pk[2], o.w = pk[3];
    *reinterpret_cast<uint4*>(slab + (size_t)slot * 16) = o;
    slab[taps * 2048 + slot] = (uint8_t)(E + 127);
  }
}

template <int BM, bool HALO>
static void launch(const ConvShape& s, const void* x, const void* w, const F8Epi& e, void* y,
                   bool out_bf16, hipStream_t st) {
  const int M = s.N * s.OH * s.OW;
  const dim3 grid((unsigned)(((M + BM - 1) / BM) * (s.K / BN)));
  const uint8_t* x8 = reinterpret_cast<const uint8_t*>(x);
  const uint8_t* w8 = reinterpret_cast<const uint8_t*>(w);
  if (out_bf16)
    mx4conv_kernel<BM, false, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
  else
    mx4conv_kernel<BM, true, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
}

#undef MX_KERNEL
#undef MX_DEV
#undef MX_TARGET

}  // namespace cmx4

F8Plan mx4conv_plan(const ConvShape& s, int form) {
  if (!f8conv_ok(s)) throw std::runtime_error("mx4conv: unsupported shape");
  if (form < 0 || form > 2) throw std::runtime_error("mx4conv: form must be 0, 1 (gather) or 2 (halo)");
  F8Plan p;
  const long long M = (long long)s.N * s.OH * s.OW;
  p.bm = (M / 128) * (s.K / 64) >= 256 ? 128 : 64;  // f8conv's rule
  const bool halo_ok = s.R == 3 && s.S == 3 && s.stride == 1 && s.pad == 1 &&
                       p.bm + 2 * s.W + 2 <= cmx4::HCAP;
  p.form = form == 0 ? (halo_ok ? 2 : 1) : form;
  if (p.form == 2 && !halo_ok)
    throw std::runtime_error("mx4conv: the halo form takes 3x3 / stride 1 / pad 1 with "
                             "bm + 2 W + 2 <= 248");
  return p;
}

void mx4conv(const ConvShape& s, const void* x, const void* w, const F8Epi& e, void* y,
             bool out_bf16, int form, hipStream_t st) {
  const F8Plan p = mx4conv_plan(s, form);
  if (!x || !w || !y || !e.a2 || !e.b || (e.res && !e.s_res) || (!out_bf16 && !e.inv_s_out))
    throw std::runtime_error("mx4conv: null operand");
  const bool halo = p.form == 2;
  if (p.bm == 128)
    halo ? cmx4::launch<128, true>(s, x, w, e, y, out_bf16, st)
         : cmx4::launch<128, false>(s, x, w, e, y, out_bf16, st);
  else
    halo ? cmx4::launch<64, true>(s, x, w, e, y, out_bf16, st)
         : cmx4::launch<64, false>(s, x, w, e, y, out_bf16, st);
}

void wq_mx4(const long long* jobs, int njobs, long long nblocks, hipStream_t st) {
  if (njobs <= 0 || nblocks <= 0 || !jobs) throw std::runtime_error("wq_mx4: bad job table");
  cmx4::wq_mx4_kernel<<<(unsigned)nblocks, cmx4::NT, 0, st>>>(jobs, njobs);
}

}  // namespace gops
