// Split-operand bf16 ("bf16x3") MFMA implicit-GEMM forward convolution for
// ResNet-18 inference at fp32-class accuracy (docs/ACCURACY.md "ResNet-18
// bf16x3 inference"), and the kernels that make its operands.
//
// Every fp32 value v travels as a pair of bf16 values, hi = bf16_rne(v) and lo
// = bf16_rne(v - hi) (v - hi is exact in fp32, hi + lo is exact in fp32, |v -
// (hi + lo)| <= 2^-16 |v|).  A split tensor is two plain bf16 planes of the
// tensor's shape, hi then lo, numel elements apart: activations NHWC, weights
// [tap][k][c] with c contiguous (wsplit_x3).  A product x w is three bf16 MFMA
// products into one fp32 accumulator, xh wh + xh wl + xl wh (each exact in
// fp32; xl wl, under 2^-16 |x w|, is dropped): the bf16 MFMA rate at a third,
// where v_mfma_f32_32x32x2_f32 runs at a sixteenth.
//
// x3conv_kernel:
//   * lowp_conv_core.h's geometry (256 threads, 2 x 2 waves, block tiles 128 x
//     64 and 64 x 64 - x3conv_plan, by M - no split-K, no atomics) and its halo
//     mask and zero row; the loaders are this file's own (32-row passes, two
//     planes, the swizzle, the stem), and so are the kernel's block and lane
//     coordinates (docs/PERF_NOTES.md: with the core's Tile the halo form
//     measured 0.7 % slower);
//   * a K tile is one tap x 32 channels = ONE 128-byte LDS row per pixel (A) and
//     per output channel (B): 16-byte pieces 0-3 are the 32 hi channels, pieces
//     4-7 the 32 lo channels.  The loaders fetch piece p of a row from plane
//     p >> 2 at channel 8 (p & 3): thread t of a 32-row pass owns row t >> 3,
//     piece t & 7, so eight lanes read 64 contiguous bytes of each plane;
//   * lane (r, h) of a wave reads, per K step c in {0, 1}, hi piece 2 c + h and
//     lo piece 4 + 2 c + h of row r of A and of B (ds_read_b128) and issues
//     v_mfma_f32_32x32x16_bf16 on (Ah, Bh), (Ah, Bl), (Al, Bh): 6 MFMAs a row
//     tile and K tile.  Both operands use the SAME slot-to-k mapping, and the
//     two lane groups cover a K step once, so the sum does not depend on the
//     hardware's k order inside a lane;
//   * swizzle.  Piece p of row j lives in slot p ^ ((j >> 1) & 7).  A
//     ds_read_b128 is served 16 lanes a cycle over 64 banks x 4 B = 256 B, and
//     the 16 lanes are 16 consecutive rows at one piece p.  With a 128-byte
//     pitch row j starts at bank 32 (j & 1): rows of one parity share 32 banks
//     = 8 slots, and the 8 such rows among 16 consecutive ones have 8
//     consecutive values of j >> 1, so their slots p ^ ((j >> 1) & 7) are a
//     permutation of 0..7: every 16-byte unit of the 256 B is hit once, for any
//     p.  Piece p and piece p + 4, read back to back, are two such reads (p + 4
//     only flips bit 2 of every slot).  The halo loader's taps read rows j +
//     shift for 16 consecutive j - still 16 consecutive rows.  The loaders'
//     ds_write_b128 (2 rows x 8 pieces a 16-lane group) fill the 16 units once
//     too.  No padding: an LDS row is exactly the 128 bytes it carries;
//   * 16-byte global loads through registers, double-buffered LDS, the next
//     tile's loads in flight during this tile's MFMAs, one barrier a K tile (a
//     small chunk fills few CUs on layer 4; that is accepted).
// Three loaders (template MODE):
//   gather  R in {1, 3}, stride in {1, 2}: each K tile gathers its BM input
//           pixels of one tap (zeros outside the image); K tiles tap-major;
//           LDS 2 (BM + 64) rows = 48 KiB at BM = 128, 32 KiB at 64;
//   halo    3x3 / stride 1 / pad 1: per 32-channel chunk the contiguous run of
//           input pixels from one image row above the block's output pixels to
//           one below (BM + 2 W + 2 <= 248 rows) is staged once, double-
//           buffered, and the nine taps read their A fragments from it at a
//           per-lane shifted row (taps outside the image read a zero row); K
//           tiles chunk-major.  conv3_kernel's idea on these rows.  LDS 2 x 249
//           + 2 x 64 rows = 80,128 bytes (78.25 KiB), two blocks a CU;
//   stem    the 4x4 / stride 1 / pad 0 conv over the 16-channel space-to-depth
//           image (s2d_stem_input_x3) with the 8x8-extended filter [k][256]
//           (s2d_stem_weight_x3): K tile kt = window row kt >> 1, the two
//           horizontally adjacent s2d pixels 2 (kt & 1), 2 (kt & 1) + 1 = 32
//           contiguous elements of each plane, always inside the padded image;
//           8 K tiles.  LDS as gather.
// The epilogue (X3Epi), fp32, in this order: v = fmaf(acc, a[k], b[k]); v +=
// hi + lo of res[m][k] (optional); ReLU; store split(v) into the two planes.
#include "lowp_conv_core.h"

namespace gops {
namespace cx3 {

using namespace lowp;

constexpr int ROW = 128;  // bytes of an LDS row: 32 hi + 32 lo channels
constexpr int HLD = (HCAP + 31) / 32;  // halo 16-byte loads a thread
enum { GATHER = 0, HALO = 1, STEM = 2 };

typedef __bf16 bf16v8 __attribute__((ext_vector_type(8)));

LOWP_DEV float bf_f32(uint32_t bits) { return __builtin_bit_cast(float, bits << 16); }
// split(v): the bits of hi = bf16_rne(v) and of lo = bf16_rne(v - hi)
LOWP_DEV void split(float v, uint32_t& hi, uint32_t& lo) {
  const __bf16 h = (__bf16)v;
  const __bf16 l = (__bf16)(v - (float)h);
  hi = __builtin_bit_cast(uint16_t, h), lo = __builtin_bit_cast(uint16_t, l);
}
// byte offset of piece p of LDS row j
LOWP_DEV int slot(int j, int p) { return j * ROW + 16 * (p ^ ((j >> 1) & 7)); }

// The operand tiles of K tile kt: load() issues the global loads into
// registers, store() writes them into the LDS buffers tile kt is read from.
// Every load is unconditional, from a pixel clamped into the tensor, and a
// pixel outside the image is zeroed in registers (no branch around a load).
// LDS: two A images of ASZ bytes, then two B tiles.
template <int BM, int MODE>
struct Loader {
  static constexpr int AR = BM / 32;
  static constexpr int ASZ = (MODE == HALO ? HCAP + 1 : BM) * ROW;
  static constexpr int BSZ = BN * ROW;
  const ConvShape s;
  const uint16_t* xp;     // this thread's plane of x, at its 8 channels of a chunk
  const uint16_t* wb[2];  // its 16 bytes of B rows lrow, lrow + 32 at (tap 0, channel 0)
  int M, cpt, lrow, pc;
  // gather / stem: the input pixel of tap (0, 0) of this thread's AR rows
  const uint16_t* xb[AR];
  int iy0[AR], ix0[AR];
  uint4 ra[MODE == HALO ? 1 : AR];
  // halo: the first pixel of the run, its rows
  long long p0;
  int hr;
  uint4 rh[MODE == HALO ? HLD : 1];
  uint4 rb[2];

  LOWP_DEV Loader(const ConvShape& s_, const uint16_t* x, const uint16_t* wt, int m0, int n0)
      : s(s_) {
    const int tid = threadIdx.x;
    M = s.N * s.OH * s.OW, cpt = s.C / 32, lrow = tid >> 3, pc = tid & 7;
    const int plane = pc >> 2, eo = 8 * (pc & 3);
    const size_t wrow = (size_t)(MODE == STEM ? s.R * s.S * s.C : s.C);
    xp = x + (size_t)plane * s.N * s.H * s.W * s.C + eo;
    const uint16_t* wp = wt + (size_t)plane * s.R * s.S * s.K * s.C + eo;
    wb[0] = wp + (size_t)(n0 + lrow) * wrow;
    wb[1] = wp + (size_t)(n0 + lrow + 32) * wrow;
    if constexpr (MODE == HALO) {
      p0 = (long long)m0 - s.W - 1;
      hr = BM + 2 * s.W + 2;
    } else {
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int m = m0 + lrow + 32 * i;
        const int mm = m < M ? m : M - 1;
        const int ox = mm % s.OW, t = mm / s.OW, oy = t % s.OH, n = t / s.OH;
        if constexpr (MODE == STEM) {  // (a row past M repeats row M - 1; it is never stored)
          xb[i] = xp + (((size_t)n * s.H + oy) * s.W + ox) * 16;
        } else if (m < M) {
          iy0[i] = oy * s.stride - s.pad, ix0[i] = ox * s.stride - s.pad;
          xb[i] = xp + (size_t)n * s.H * s.W * s.C;
        } else {  // a row past M: every tap is outside
          iy0[i] = -(1 << 20), ix0[i] = 0, xb[i] = xp;
        }
      }
    }
  }
  LOWP_DEV void load(int kt) {
    size_t wo;
    if constexpr (MODE == HALO) {
      const int chunk = kt / 9, tap = kt - 9 * chunk, c0 = chunk * 32;
      wo = (size_t)tap * s.K * s.C + c0;
      if (tap == 0) {
#pragma unroll
        for (int i = 0; i < HLD; ++i) {
          const long long p = p0 + lrow + 32 * i, q = p < 0 ? 0 : (p < M ? p : M - 1);
          rh[i] = keep4(*reinterpret_cast<const uint4*>(xp + (size_t)q * s.C + c0), p == q);
        }
      }
    } else if constexpr (MODE == STEM) {
      wo = 32 * kt;
      const size_t ao = ((size_t)(kt >> 1) * s.W + 2 * (kt & 1)) * 16;
#pragma unroll
      for (int i = 0; i < AR; ++i) ra[i] = *reinterpret_cast<const uint4*>(xb[i] + ao);
    } else {
      const int tap = kt / cpt, c0 = (kt - tap * cpt) * 32;
      const int kh = tap / s.S, kw = tap - kh * s.S;
      wo = (size_t)tap * s.K * s.C + c0;
#pragma unroll
      for (int i = 0; i < AR; ++i) {
        const int iy = iy0[i] + kh, ix = ix0[i] + kw;
        const int yc = min(max(iy, 0), s.H - 1), xc = min(max(ix, 0), s.W - 1);
        ra[i] = keep4(*reinterpret_cast<const uint4*>(xb[i] + ((size_t)yc * s.W + xc) * s.C + c0),
                      iy == yc && ix == xc);
      }
    }
    rb[0] = *reinterpret_cast<const uint4*>(wb[0] + wo);
    rb[1] = *reinterpret_cast<const uint4*>(wb[1] + wo);
  }
  LOWP_DEV void store(int kt, char* smem) const {
    if constexpr (MODE == HALO) {
      const int chunk = kt / 9;
      if (kt - 9 * chunk == 0) {
        char* A = smem + (chunk & 1) * ASZ;
#pragma unroll
        for (int i = 0; i < HLD; ++i) {
          const int j = lrow + 32 * i;
          if (j < hr) *reinterpret_cast<uint4*>(A + slot(j, pc)) = rh[i];
        }
      }
    } else {
      char* A = smem + (kt & 1) * ASZ;
#pragma unroll
      for (int i = 0; i < AR; ++i) *reinterpret_cast<uint4*>(A + slot(lrow + 32 * i, pc)) = ra[i];
    }
    char* B = smem + 2 * ASZ + (kt & 1) * BSZ;
    *reinterpret_cast<uint4*>(B + slot(lrow, pc)) = rb[0];
    *reinterpret_cast<uint4*>(B + slot(lrow + 32, pc)) = rb[1];
  }
};

// this lane's fragments of LDS row j: hi pieces h, 2 + h and lo pieces 4 + h, 6 + h
struct Frag {
  bf16v8 hi[2], lo[2];
};
LOWP_DEV Frag frag(const char* base, int j, int h) {
  Frag f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    f.hi[c] = __builtin_bit_cast(bf16v8, *reinterpret_cast<const uint4*>(base + slot(j, 2 * c + h)));
    f.lo[c] =
        __builtin_bit_cast(bf16v8, *reinterpret_cast<const uint4*>(base + slot(j, 4 + 2 * c + h)));
  }
  return f;
}
// one K tile of a 32 x 32 accumulator: per K step (Ah, Bh), (Ah, Bl), (Al, Bh)
LOWP_DEV f32x16 mma_tile(const Frag& a, const Frag& b, f32x16 acc) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi[c], b.hi[c], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi[c], b.lo[c], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo[c], b.hi[c], acc, 0, 0, 0);
  }
  return acc;
}

template <int BM, int MODE>
LOWP_KERNEL(NT) void x3conv_kernel(const ConvShape s, const uint16_t* __restrict__ x,
                                   const uint16_t* __restrict__ wt, const X3Epi e,
                                   uint16_t* __restrict__ y) {
  using LD = Loader<BM, MODE>;
  constexpr int TM = BM / 64;
  constexpr int ASZ = LD::ASZ, BSZ = LD::BSZ;
  __shared__ __attribute__((aligned(16))) char smem[2 * ASZ + 2 * BSZ];
  const int M = s.N * s.OH * s.OW;
  const int mt = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (bid % mt) * BM, n0 = (bid / mt) * BN;
  const int nk = MODE == STEM ? 8 : s.R * s.S * (s.C / 32);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
  const int r = lane & 31, h = lane >> 5;
  LD ld(s, x, wt, m0, n0);
  // the epilogue's per-column operands, loaded before the main loop
  // (fwd_kernel: a load behind the first stores would wait for them)
  const int co = n0 + wn * 32 + r;
  const float fa = e.a[co], fb = e.b[co];
  int mask[TM];
  if constexpr (MODE == HALO) {
    zero_halo_rows(smem, ASZ, ROW);
#pragma unroll
    for (int i = 0; i < TM; ++i) mask[i] = halo_mask(s, m0 + wm * (BM / 2) + 32 * i + r, M);
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
    const Frag b = frag(smem + 2 * ASZ + (kt & 1) * BSZ, wn * 32 + r, h);
    if constexpr (MODE == HALO) {
      const int chunk = kt / 9, tap = kt - 9 * chunk;
      const int shift = (tap / 3) * s.W + tap % 3;
      const char* A = smem + (chunk & 1) * ASZ;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = (mask[i] >> tap) & 1 ? wm * (BM / 2) + 32 * i + r + shift : HCAP;
        acc[i] = mma_tile(frag(A, row, h), b, acc[i]);
      }
    } else {
      const char* A = smem + (kt & 1) * ASZ;
#pragma unroll
      for (int i = 0; i < TM; ++i)
        acc[i] = mma_tile(frag(A, wm * (BM / 2) + 32 * i + r, h), b, acc[i]);
    }
    if (more) ld.store(kt + 1, smem);
    block_sync();
  }
  // lane (r, h) holds column co of rows mb + (q & 3) + 8 (q >> 2); the residual
  // planes load first (rows clamped into the tensor), the stores last
  const uint16_t* res = reinterpret_cast<const uint16_t*>(e.res);
  const size_t K = s.K, MK = (size_t)M * K;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int mb = m0 + wm * (BM / 2) + 32 * i + 4 * h;
    float rv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const size_t at = (size_t)min(mb + (q & 3) + 8 * (q >> 2), M - 1) * K + co;
      rv[q] = res ? bf_f32(res[at]) + bf_f32(res[MK + at]) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = mb + (q & 3) + 8 * (q >> 2);
      float v = __builtin_fmaf(acc[i][q], fa, fb);
      if (res) v += rv[q];
      if (e.relu) v = fmaxf(v, 0.f);
      if (m >= M) continue;
      uint32_t hi, lo;
      split(v, hi, lo);
      y[(size_t)m * K + co] = (uint16_t)hi;
      y[MK + (size_t)m * K + co] = (uint16_t)lo;
    }
  }
}

// n fp32 values into the planes out[0, n) (hi) and out[n, 2 n) (lo): eight
// values a thread from two 16-byte loads into one 16-byte store a plane (the lo
// plane starts 2 n bytes in: for n % 8 != 0 its stores are scalar), the n % 8
// tail by the first threads of block 0.
LOWP_KERNEL(NT) void split_kernel(const float* __restrict__ x, long long n, uint16_t* __restrict__ out) {
  const long long n8 = n / 8, stride = (long long)gridDim.x * NT;
  const bool lo16 = n % 8 == 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n8; i += stride) {
    const float4 u = reinterpret_cast<const float4*>(x)[2 * i];
    const float4 v = reinterpret_cast<const float4*>(x)[2 * i + 1];
    const float f[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    uint32_t hi[8], lo[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) split(f[c], hi[c], lo[c]);
    uint4 ph, pl;
    ph.x = hi[0] | hi[1] << 16, ph.y = hi[2] | hi[3] << 16, ph.z = hi[4] | hi[5] << 16,
    ph.w = hi[6] | hi[7] << 16;
    pl.x = lo[0] | lo[1] << 16, pl.y = lo[2] | lo[3] << 16, pl.z = lo[4] | lo[5] << 16,
    pl.w = lo[6] | lo[7] << 16;
    reinterpret_cast<uint4*>(out)[i] = ph;
    if (lo16) {
      reinterpret_cast<uint4*>(out + n)[i] = pl;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) out[n + 8 * i + c] = (uint16_t)lo[c];
    }
  }
  const long long t = 8 * n8 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    uint32_t hi, lo;
    split(x[t], hi, lo);
    out[t] = (uint16_t)hi, out[n + t] = (uint16_t)lo;
  }
}

// Every conv's weights in ONE launch: jobs[j] = {w (HWIO fp32), out (bf16
// planes [2][tap][k][c]), taps, C, K, 0, first block, 0} (int64), K / 32 blocks
// a job, first blocks ascending.  A block owns 32 output channels and walks
// their slice 32 x 32 at a time through an LDS transpose, c contiguous on the
// way out, into both planes.
LOWP_KERNEL(NT) void wsplit_kernel(const long long* __restrict__ jobs, int njobs) {
  __shared__ float t[32][33];
  const int b = blockIdx.x;
  int j = 0;
  for (int i = 1; i < njobs; ++i)
    if (jobs[8 * i + 6] <= b) j = i;
  const long long* J = jobs + 8 * j;
  const float* w = reinterpret_cast<const float*>(J[0]);
  uint16_t* out = reinterpret_cast<uint16_t*>(J[1]);
  const int taps = (int)J[2], C = (int)J[3], K = (int)J[4];
  const size_t plane = (size_t)taps * K * C;
  const int k0 = (b - (int)J[6]) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int tap = 0; tap < taps; ++tap)
    for (int c0 = 0; c0 < C; c0 += 32) {
      const float* src = w + ((size_t)tap * C + c0) * K + k0;
#pragma unroll
      for (int i = 0; i < 4; ++i) t[ty + 8 * i][tx] = src[(size_t)(ty + 8 * i) * K + tx];
      block_sync();
      uint16_t* dst = out + ((size_t)tap * K + k0) * C + c0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = ty + 8 * i;
        uint32_t hi, lo;
        split(t[tx][k], hi, lo);
        dst[(size_t)k * C + tx] = (uint16_t)hi;
        dst[plane + (size_t)k * C + tx] = (uint16_t)lo;
      }
      block_sync();
    }
}

// The split forms of s2d_stem_input / s2d_stem_weight (ops_generic.hip; the
// layouts are theirs): one thread per s2d pixel (n, Y, X) of [N][Hs][Ws],
// channels (p * 2 + q) * 3 + ci = x[n][2 (Y - 2) + p][2 (X - 2) + q][ci] (zero
// outside the image), 4 zero channels; two 16-byte stores a plane.
LOWP_KERNEL(NT) void s2d_input_kernel(const float* __restrict__ x, int N, int H, int W, int Hs, int Ws,
                                uint4* __restrict__ xs) {
  const long long n_pix = (long long)N * Hs * Ws;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n_pix;
       i += (long long)gridDim.x * NT) {
    const int X = (int)(i % Ws);
    const long long t = i / Ws;
    const int Y = (int)(t % Hs), n = (int)(t / Hs);
    uint32_t hi[16], lo[16];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int iy = 2 * (Y - 2) + p;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int ix = 2 * (X - 2) + q;
        const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float* src = x + (((size_t)n * H + (ok ? iy : 0)) * W + (ok ? ix : 0)) * 3;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const int c = (p * 2 + q) * 3 + ci;
          split(ok ? src[ci] : 0.f, hi[c], lo[c]);
        }
      }
    }
#pragma unroll
    for (int c = 12; c < 16; ++c) hi[c] = lo[c] = 0u;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const uint32_t* a = hi + 8 * half;
      const uint32_t* b = lo + 8 * half;
      uint4 ph, pl;
      ph.x = a[0] | a[1] << 16, ph.y = a[2] | a[3] << 16, ph.z = a[4] | a[5] << 16,
      ph.w = a[6] | a[7] << 16;
      pl.x = b[0] | b[1] << 16, pl.y = b[2] | b[3] << 16, pl.z = b[4] | b[5] << 16,
      pl.w = b[6] | b[7] << 16;
      xs[2 * i + half] = ph;
      xs[2 * (n_pix + i) + half] = pl;
    }
  }
}

// wt8 planes [2][co][k], k = (a * 4 + b) * 16 + (p * 2 + q) * 3 + ci  <-
// w[2a + p - 1][2b + q - 1][ci][co] (zero off the 7x7 kernel and on the 4
// padding channels)
LOWP_KERNEL(NT) void s2d_weight_kernel(const float* __restrict__ w, int K, uint16_t* __restrict__ wt8) {
  const int n = K * 256;
  for (int i = blockIdx.x * NT + threadIdx.x; i < n; i += gridDim.x * NT) {
    const int co = i >> 8, k = i & 255, tap = k >> 4, ch = k & 15;
    const int a = tap >> 2, b = tap & 3, pq = ch / 3, ci = ch - 3 * pq;
    const int ky = 2 * a + (pq >> 1) - 1, kx = 2 * b + (pq & 1) - 1;
    const bool ok = ch < 12 && ky >= 0 && ky < 7 && kx >= 0 && kx < 7;
    uint32_t hi, lo;
    split(ok ? w[((size_t)(ky * 7 + kx) * 3 + ci) * K + co] : 0.f, hi, lo);
    wt8[i] = (uint16_t)hi, wt8[n + i] = (uint16_t)lo;
  }
}

template <int BM, int MODE>
static void launch(const ConvShape& s, const void* x, const void* w, const X3Epi& e, void* y,
                   hipStream_t st) {
  x3conv_kernel<BM, MODE><<<conv_grid(s, BM), NT, 0, st>>>(
      s, reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(w), e,
      reinterpret_cast<uint16_t*>(y));
}

static inline int grid1d(long long n) {
  const long long b = (n + NT - 1) / NT;
  return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}

}  // namespace cx3

static bool x3_stem_shape(const ConvShape& s) {
  return s.R == 4 && s.S == 4 && s.C == 16 && s.stride == 1 && s.pad == 0;
}

bool x3conv_ok(const ConvShape& s) {
  const long long M = (long long)s.N * s.OH * s.OW;
  const bool stem = x3_stem_shape(s);
  const bool conv = s.R == s.S && (s.R == 1 || s.R == 3) && (s.stride == 1 || s.stride == 2) &&
                    s.pad >= 0 && s.pad < s.R && s.C >= 32 && s.C % 32 == 0;
  return (stem || conv) && s.K >= 64 && s.K % 64 == 0 && s.N >= 1 &&
         s.OH == (s.H + 2 * s.pad - s.R) / s.stride + 1 &&
         s.OW == (s.W + 2 * s.pad - s.R) / s.stride + 1 && s.OH >= 1 && s.OW >= 1 &&
         M + 128 < (1LL << 31) && (long long)s.N * s.H * s.W < (1LL << 31);
}

X3Plan x3conv_plan(const ConvShape& s, int form) {
  if (!x3conv_ok(s)) throw std::runtime_error("x3conv: unsupported shape");
  if (form < 0 || form > 3)
    throw std::runtime_error("x3conv: form must be 0, 1 (gather), 2 (halo) or 3 (stem)");
  X3Plan p;
  const long long M = (long long)s.N * s.OH * s.OW;
  // the M rule: 128-row tiles (each B fragment feeds two accumulators) once 64
  // of them exist; below that, 64-row tiles for the blocks
  p.bm = M >= 128 * 64 ? 128 : 64;
  const bool stem = x3_stem_shape(s);
  p.form = form ? form : stem ? 3 : lowp::halo_ok(s, p.bm) ? 2 : 1;
  if ((p.form == 3) != stem)
    throw std::runtime_error("x3conv: the stem form takes the 4x4 / stride 1 / pad 0 conv over 16 "
                             "channels, and that conv takes no other form");
  if (p.form == 2 && !lowp::halo_ok(s, p.bm))
    throw std::runtime_error("x3conv: the halo form takes 3x3 / stride 1 / pad 1 with "
                             "bm + 2 W + 2 <= 248");
  return p;
}

void x3conv(const ConvShape& s, const void* x, const void* w, const X3Epi& e, void* y, int form,
            hipStream_t st) {
  const X3Plan p = x3conv_plan(s, form);
  if (!x || !w || !y || !e.a || !e.b) throw std::runtime_error("x3conv: null operand");
#define X3_GO(BM)                                                                   \
  (p.form == 3   ? cx3::launch<BM, cx3::STEM>(s, x, w, e, y, st)                    \
   : p.form == 2 ? cx3::launch<BM, cx3::HALO>(s, x, w, e, y, st)                    \
                 : cx3::launch<BM, cx3::GATHER>(s, x, w, e, y, st))
  if (p.bm == 128)
    X3_GO(128);
  else
    X3_GO(64);
#undef X3_GO
}

void x3_split(const float* x, long long n, void* planes, hipStream_t st) {
  if (n < 1 || !x || !planes) throw std::runtime_error("x3_split: empty buffer");
  cx3::split_kernel<<<cx3::grid1d(n / 8), cx3::NT, 0, st>>>(x, n,
                                                            reinterpret_cast<uint16_t*>(planes));
}

void wsplit_x3(const long long* jobs, int njobs, long long nblocks, hipStream_t st) {
  if (njobs <= 0 || nblocks <= 0 || !jobs) throw std::runtime_error("wsplit_x3: bad job table");
  cx3::wsplit_kernel<<<(unsigned)nblocks, cx3::NT, 0, st>>>(jobs, njobs);
}

void s2d_stem_input_x3(const float* x, int N, int H, int W, int OH, int OW, void* xs,
                       hipStream_t st) {
  const long long n = (long long)N * (OH + 3) * (OW + 3);
  cx3::s2d_input_kernel<<<cx3::grid1d(n), cx3::NT, 0, st>>>(x, N, H, W, OH + 3, OW + 3,
                                                            reinterpret_cast<uint4*>(xs));
}

void s2d_stem_weight_x3(const float* w, int K, void* wt8, hipStream_t st) {
  cx3::s2d_weight_kernel<<<cx3::grid1d((long long)K * 256), cx3::NT, 0, st>>>(
      w, K, reinterpret_cast<uint16_t*>(wt8));
}

}  // namespace gops
