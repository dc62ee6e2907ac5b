// OCP microscaling FP4 (MXFP4) weights x e4m3 activations: the MFMA implicit-
// GEMM forward convolution of ResNet-18 --dtype mxfp4 inference
// (docs/ACCURACY.md "ResNet-18 mxfp4 inference"), and the weight quantiser that
// feeds it.
//
// lowp_conv_core.h's geometry (256 threads, 2 x 2 waves, block tiles 128 x 64
// and 64 x 64 by byte_conv_plan's rule, no split-K, no atomics), its A loaders
// (HaloA, GatherA) and its epilogue (F8Epi), all shared with conv_f8.hip; the B
// operand and the K loop are this file's own.
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
//   halo    3x3 / stride 1 / pad 1 (halo_ok): A is the core's halo image
//           (pitch 80, a zero row, per-lane tap masks), double-buffered;
//           the 9-tap slab (19,584 bytes) is single-buffered.  Per chunk the
//           next chunk's halo and slab loads are issued into registers, the
//           nine taps run back to back from LDS with no barrier between them,
//           then the halo registers go to the other image, a barrier, the slab
//           registers over the slab, a barrier: two barriers a chunk where
//           f8conv takes nine.  LDS 39,840 + 19,584 bytes (static).
//   gather  R in {1, 3}, stride in {1, 2}: the core's per-tap gathered A tile,
//           double-buffered, one barrier a tap; A tiles are small here, so the
//           slab is double-buffered too (20,480 + 39,168 bytes at BM = 128) and
//           a 1x1 conv keeps one barrier a K tile.
#include "lowp_conv_core.h"

namespace gops {
namespace cmx4 {

using namespace lowp;

constexpr int TAPB = 2048 + 128;  // slab bytes a tap: codes, scales
constexpr int SLAB9 = 9 * TAPB;
constexpr int SLD = (SLAB9 / 16 + NT - 1) / NT;  // slab 16-byte loads a thread

typedef int i32x8 __attribute__((ext_vector_type(8)));

// The slab of one chunk: load() issues this thread's 16-byte global loads,
// store() writes them to an LDS slab.  n16 = taps * 136 vectors.
struct Slab {
  u32x4 rs[SLD];
  LOWP_DEV void load(const uint8_t* g, int n16) {
#pragma unroll
    for (int i = 0; i < SLD; ++i) {
      const int j = threadIdx.x + NT * i;
      rs[i] = reinterpret_cast<const u32x4*>(g)[j < n16 ? j : 0];
    }
  }
  LOWP_DEV void store(char* lds, int n16) const {
#pragma unroll
    for (int i = 0; i < SLD; ++i) {
      const int j = threadIdx.x + NT * i;
      if (j < n16) reinterpret_cast<u32x4*>(lds)[j] = rs[i];
    }
  }
};

// one (tap, chunk) of a 32 x 32 accumulator: the lane's two 16-byte runs of A
// (ap = its row + 16 h), its 16 bytes of B codes and its block scale
LOWP_DEV f32x16 mma_tile(const char* ap, const uint4 b, int scale, f32x16 acc) {
  const uint4 a0 = *reinterpret_cast<const uint4*>(ap);
  const uint4 a1 = *reinterpret_cast<const uint4*>(ap + 32);
  const i32x8 av = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w,
                    (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
  const i32x8 bv = {(int)b.x, (int)b.y, (int)b.z, (int)b.w, 0, 0, 0, 0};
  // cbsz 0: A e4m3, scale 2^0; blgp 4: B e2m1, scale byte 0 of `scale`
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 4, 0, 0x7f7f7f7f, 0, scale);
}

// (two waves a SIMD: the two blocks a CU's LDS holds)
template <int BM, bool OUT8, bool HALO>
LOWP_KERNEL(NT, 2) void mx4conv_kernel(const ConvShape s, const uint8_t* __restrict__ x,
                                       const uint8_t* __restrict__ wt, const F8Epi e,
                                       void* __restrict__ yv) {
  constexpr int TM = BM / 64;
  constexpr int ASZ = HALO ? HaloA<BM>::ASZ : GatherA<BM>::ASZ;
  __shared__ __attribute__((aligned(16))) char smem[2 * ASZ + (HALO ? 1 : 2) * SLAB9];
  char* const sl = smem + 2 * ASZ;
  const Tile<BM> t(s);
  const int taps = s.R * s.S, nch = s.C / BK;
  const int n16 = taps * (TAPB / 16);
  const int lane = threadIdx.x & 63, h = t.h;
  // this block's slabs: chunk ch at ws + ch * taps * TAPB
  const uint8_t* ws = wt + (size_t)(t.n0 / BN) * nch * taps * TAPB;
  // this lane's B codes and scale byte of tap 0 inside a slab
  const int bo = t.wn * 1024 + lane * 16, so = taps * 2048 + t.wn * 64 + lane;
  // the epilogue's operands, loaded before the main loop
  const float fa = e.a2[t.co], fb = e.b[t.co];
  const float sres = e.res ? *e.s_res : 0.f;
  const float inv = OUT8 ? *e.inv_s_out : 1.f;
  f32x16 acc[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) acc[i] = zero16();
  Slab sb;
  if constexpr (HALO) {
    zero_halo_rows(smem, ASZ, PITCH);
    int mask[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) mask[i] = halo_mask(s, t.m0 + t.row(i), t.M);
    HaloA<BM> ha(s, x, t.m0);
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
            const int row = (mask[i] >> tap) & 1 ? t.row(i) + shift : HCAP;
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
    GatherA<BM> ga(s, x, t.m0);
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
        for (int i = 0; i < TM; ++i) acc[i] = mma_tile(A + t.row(i) * PITCH, b, sc, acc[i]);
        if (more) ga.store(smem + ((kt + 1) & 1) * ASZ);
        // the other slab: its readers passed the barrier that ended chunk ch - 1
        if (last && more) sb.store(sl + ((ch + 1) & 1) * SLAB9, n16);
        block_sync();
      }
    }
  }
  f8_epilogue<BM, OUT8>(acc, e, fa, fb, sres, inv, t, (size_t)s.K, yv);
}

// E of a block: the least integer with 6 2^E >= amax, 0 for an all-zero block,
// held to [-100, 100].  Exact: amax = m 2^e with m in [0.5, 1) and 6 = 0.75
// 2^3, so E = e - 3 for m <= 0.75, else e - 2.
LOWP_DEV int block_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int ex;
  const float m = frexpf(amax, &ex);
  return min(max(m <= 0.75f ? ex - 3 : ex - 2, -100), 100);
}

// e2m1 code of v = w 2^-E (exact): the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6},
// a tie to the even 3-bit magnitude index; w's sign in bit 3
LOWP_DEV uint32_t e2m1(float w, float inv) {
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
LOWP_KERNEL(NT, 2) void wq_mx4_kernel(const long long* __restrict__ jobs, int njobs) {
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
  const dim3 grid = conv_grid(s, BM);
  const uint8_t* x8 = reinterpret_cast<const uint8_t*>(x);
  const uint8_t* w8 = reinterpret_cast<const uint8_t*>(w);
  if (out_bf16)
    mx4conv_kernel<BM, false, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
  else
    mx4conv_kernel<BM, true, HALO><<<grid, NT, 0, st>>>(s, x8, w8, e, y);
}

}  // namespace cmx4

// form 0: the halo form wherever it applies
F8Plan mx4conv_plan(const ConvShape& s, int form) {
  return lowp::byte_conv_plan(s, form, 2, "mx4conv");
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
