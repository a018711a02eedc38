// CKKS encode / decode on the device (fhe_encode / fhe_decode): the special FFT over the rotation
// group in float64, the lift of the rounded coefficients into residues, and the two-limb centring
// of a plaintext back into doubles.  tests/encode_ref.py restates every step; the results agree
// with it bit for bit, which needs each butterfly to be exactly
//   (dr wr - di wi, dr wi + di wr)   four rounded products, two rounded sums
// so this translation unit is compiled with floating-point contraction off (no FMA).
//
// Organisation.  n = N / 2 complex points per plaintext, 16 bytes each.  One workgroup runs up to
// kTileLog radix-2 stages on a tile of 2^kTileLog points in LDS (32 KiB).  n <= 2^kTileLog
// (N <= 2^12): one pass.  Above: two passes over a workspace [count][n] that stays in cache
//   strided     the top ln - kTileLog stages; a tile is 2^B rows of 2^C contiguous points
//               (B + C = kTileLog), the rows 2^(ln - B) points apart
//   contiguous  the low kTileLog stages on 2^kTileLog consecutive points
// Encode (decimation in frequency, stages len = n .. 2) runs strided then contiguous and folds
// the bit reversal, the scaling and the rounding into the contiguous pass's stores; decode
// (decimation in time, len = 2 .. n) folds the bit reversal into the contiguous pass's loads and
// the division by delta into the strided pass's stores.
//
// Sparse packing (fhe_encode_sparse / fhe_decode_sparse, n_s < N / 2 slots) is the same network on
// n_s points with the same tables, in a kernel of its own (k_sfft_sparse, below): the dense
// kernel and its launches stay what they were.
#pragma clang fp contract(off)

#include <cmath>

#include "internal.hpp"

namespace fhe {
namespace {

constexpr int kTileLog = 11;
constexpr int kFftThreads = 256;
// LDS index of tile element e: one 16-byte pad per 16 elements, so that the power-of-two strides
// of the low stages spread over the 256-byte bank row
__device__ __forceinline__ u32 lpad(u32 e) { return e + (e >> 4); }
constexpr u32 kTileLds = (1u << kTileLog) + (1u << (kTileLog - 4));

enum InMode : int { kInComplex = 0, kInCoeff = 1 };
enum OutMode : int { kOutComplex = 0, kOutRound = 1, kOutDivide = 2 };

struct FftPass {
  const void* in;   // kInComplex: double2 [count][n]; kInCoeff: double [count][N], gathered
  void* out;        // kOutComplex / kOutDivide: double2 [count][n]; kOutRound: int64 [count][N]
  const double2* roots;  // [2N]
  const u32* rot;        // [n] 5^j mod 2N
  double scale;          // kOutRound: delta / n; kOutDivide: delta
  u32 ln;                // log2 n
  u32 T;                 // log2 of the tile
  u32 C;                 // log2 of the contiguous run of a tile row (T: the contiguous pass)
  u32 b_lo;              // global bit of the pass's lowest stage (lh = 2^b_lo)
  u32 B;                 // stages
  u32 tiles;             // tiles per plaintext, n >> T
  int in_mode, out_mode;
};

__device__ __forceinline__ u32 brev(u32 x, u32 bits) { return __brev(x) >> (32 - bits); }

// One butterfly in place: ENC (a, b) -> (a + b, (a - b) w), else (a, b) -> (a + b w, a - b w).
template <bool ENC>
__device__ __forceinline__ void butterfly(double2& a, double2& b, const double2 w) {
  const double2 x = a, y = b;
  if (ENC) {
    a = make_double2(x.x + y.x, x.y + y.y);
    const double dr = x.x - y.x, di = x.y - y.y;
    const double p1 = dr * w.x, p2 = di * w.y, p3 = dr * w.y, p4 = di * w.x;
    b = make_double2(p1 - p2, p3 + p4);
  } else {
    const double p1 = y.x * w.x, p2 = y.y * w.y, p3 = y.x * w.y, p4 = y.y * w.x;
    const double br = p1 - p2, bi = p3 + p4;
    a = make_double2(x.x + br, x.y + bi);
    b = make_double2(x.x - br, x.y - bi);
  }
}

// ENC: the inverse special FFT of encode; otherwise the forward one of decode.
template <bool ENC>
__global__ __launch_bounds__(kFftThreads) void k_sfft_pass(const FftPass a) {
  __shared__ double2 lds[kTileLds];
  const u32 tl = blockIdx.x % a.tiles, p = blockIdx.x / a.tiles;
  const u32 n = 1u << a.ln, T = a.T, C = a.C;
  const bool strided = C < T;
  // strided: tile = (hi, chunk of 2^C within the 2^b_lo low indices); rows 2^b_lo apart
  const u32 lc_bits = strided ? a.b_lo - C : 0;
  const u32 base = strided ? ((tl >> lc_bits) << (a.b_lo + a.B)) + ((tl & ((1u << lc_bits) - 1)) << C)
                           : tl << T;
  const u32 cmask = (1u << C) - 1;
  const u32 lb = strided ? C : 0;  // local bit of the pass's lowest stage
  auto gidx = [&](u32 e) { return strided ? base + ((e >> C) << a.b_lo) + (e & cmask) : base + e; };

  for (u32 e = threadIdx.x; e < (1u << T); e += kFftThreads) {
    const u32 g = gidx(e);
    double2 v;
    if (a.in_mode == kInCoeff) {
      const double* x = static_cast<const double*>(a.in) + (u64)p * 2 * n;
      const u32 k = brev(g, a.ln);
      v = make_double2(x[k], x[k + n]);
    } else {
      v = static_cast<const double2*>(a.in)[(u64)p * n + g];
    }
    lds[lpad(e)] = v;
  }
  __syncthreads();

  for (u32 st = 0; st < a.B; ++st) {
    const u32 i = ENC ? a.B - 1 - st : st;
    const u32 pb = lb + i;       // local bit of this stage's half length
    const u32 gb = a.b_lo + i;   // lh = 2^gb, lq = 8 lh
    const u32 lqm = (8u << gb) - 1, wsh = a.ln - 1 - gb;
    for (u32 k = threadIdx.x; k < (1u << (T - 1)); k += kFftThreads) {
      const u32 ea = ((k >> pb) << (pb + 1)) | (k & ((1u << pb) - 1));
      const u32 eb = ea + (1u << pb);
      const u32 j = gidx(ea) & ((1u << gb) - 1);
      const u32 r = a.rot[j] & lqm;
      const double2 w = a.roots[(ENC ? lqm + 1 - r : r) << wsh];
      butterfly<ENC>(lds[lpad(ea)], lds[lpad(eb)], w);
    }
    __syncthreads();
  }

  for (u32 e = threadIdx.x; e < (1u << T); e += kFftThreads) {
    const u32 g = gidx(e);
    const double2 v = lds[lpad(e)];
    if (a.out_mode == kOutRound) {
      long long* c = static_cast<long long*>(a.out) + (u64)p * 2 * n;
      const u32 k = brev(g, a.ln);
      c[k] = (long long)rint(v.x * a.scale);
      c[k + n] = (long long)rint(v.y * a.scale);
    } else if (a.out_mode == kOutDivide) {
      static_cast<double2*>(a.out)[(u64)p * n + g] = make_double2(v.x / a.scale, v.y / a.scale);
    } else {
      static_cast<double2*>(a.out)[(u64)p * n + g] = v;
    }
  }
}

template <bool ENC>
int launch_pass(const FftPass& a, u32 count, hipStream_t s) {
  const u64 blocks = (u64)a.tiles * count;
  if (int rc = check_grid(blocks, kFftThreads, 1, 1, ENC ? "encode" : "decode")) return rc;
  k_sfft_pass<ENC><<<dim3((u32)blocks), kFftThreads, 0, s>>>(a);
  FHE_HIP_CHECK(hipGetLastError());
  return kOk;
}

// The special FFT of `count` plaintexts: ENC slots -> int64 coefficients [count][N] (scale =
// delta / n), else doubles [count][N] -> slots (scale = delta).  work [count][n] complex, used by
// the two-pass sizes only.
template <bool ENC>
int launch_sfft(const fhe_ctx* c, const void* in, void* out, double2* work, double scale,
                u32 count, hipStream_t s) {
  const u32 ln = c->log_n - 1;
  FftPass a{};
  a.roots = c->d_enc_roots;
  a.rot = c->d_enc_rot;
  a.scale = scale;
  a.ln = ln;
  a.T = std::min<u32>(ln, kTileLog);
  a.tiles = 1u << (ln - a.T);
  const FftPass contiguous = [&] {
    FftPass x = a;
    x.C = x.T;
    x.b_lo = 0;
    x.B = x.T;
    return x;
  }();
  if (ln <= (u32)kTileLog) {
    FftPass x = contiguous;
    x.in = in;
    x.out = out;
    x.in_mode = ENC ? kInComplex : kInCoeff;
    x.out_mode = ENC ? kOutRound : kOutDivide;
    return launch_pass<ENC>(x, count, s);
  }
  FftPass strided = a;
  strided.B = ln - kTileLog;
  strided.C = kTileLog - strided.B;
  strided.b_lo = kTileLog;
  FftPass first = ENC ? strided : contiguous, second = ENC ? contiguous : strided;
  first.in = in;
  first.out = work;
  first.in_mode = ENC ? kInComplex : kInCoeff;
  first.out_mode = kOutComplex;
  second.in = work;
  second.out = out;
  second.in_mode = kInComplex;
  second.out_mode = ENC ? kOutRound : kOutDivide;
  if (int rc = launch_pass<ENC>(first, count, s)) return rc;
  return launch_pass<ENC>(second, count, s);
}

// ---- sparse packing: n_s = 2^ls slots, ls <= log_n - 2, gap = N / (2 n_s) = 2^lg >= 2 ----------
// The transform is the same network on n_s points with the ring's own tables: rot[j] mod lq is
// 5^j mod lq whatever the ring, and W_s[k] = W[k gap], so only the twiddle shift changes
// (log_n - 2 - gb: FftPass::ln is now the slot count's logarithm and no longer gives it).
//
// One pass (ls <= kTileLog): a tile holds 2^P whole plaintexts next to each other, element
// e = (q, point); their stages are independent and share j, so the butterfly loop is the dense
// one on 2^(ls + P) elements.  The last tile may hold fewer than 2^P plaintexts (zero-filled,
// not stored).  Two passes (ls > kTileLog): P = 0 and the tiles are the dense kernel's with
// n_s for n.
//
// Encode's rounding store writes whole runs: coefficient k gap and the gap - 1 zeros behind it,
// so the coefficients [count][N] need no memset and the lift reads nothing unwritten.  The loop
// runs over the tile's *output* coefficients in ascending order (lane i -> coefficient rank i,
// the point found through the bit reversal), so a wave's 64 stores are 512 contiguous bytes
// (one pass) or whole runs (two passes, where a tile's points are 2^(ls - kTileLog) runs apart).
// A tile's outputs are 2^(P + log_n) coefficients, far more than its 2^T points: above
// 2^kStoreLog of them the store is cut into 2^S slices, one workgroup each, every one of which
// redoes the tile's (small) transform -- few workgroups writing megabytes each is what makes a
// small transform slower than the dense one otherwise.  For the same reason P stops where a
// tile's outputs reach 2^kStoreLog.
constexpr u32 kStoreLog = 13;

struct SparsePass {
  FftPass f;   // ln = ls, T = log2 of a plaintext's points in the tile, tiles = n_s >> T
  u32 wbase;   // log_n - 2: the twiddle shift of the stage lh = 2^gb is wbase - gb
  u32 lg;      // log2 gap
  u32 P;       // log2 of the plaintexts per tile
  u32 S;       // log2 of the store slices per tile (kOutRound)
  u32 count;
};

__device__ __forceinline__ u32 brev0(u32 x, u32 bits) { return bits ? brev(x, bits) : 0; }

template <bool ENC>
__global__ __launch_bounds__(kFftThreads) void k_sfft_sparse(const SparsePass sp) {
  __shared__ double2 lds[kTileLds];
  const FftPass& a = sp.f;
  const u32 n = 1u << a.ln, Tp = a.T, T = Tp + sp.P, C = a.C;
  const u32 sl = blockIdx.x & ((1u << sp.S) - 1), blk = blockIdx.x >> sp.S;
  const u32 tl = blk % a.tiles, p0 = (blk / a.tiles) << sp.P;
  const bool strided = C < Tp;
  const u32 lc_bits = strided ? a.b_lo - C : 0;
  const u32 base = strided ? ((tl >> lc_bits) << (a.b_lo + a.B)) + ((tl & ((1u << lc_bits) - 1)) << C)
                           : tl << Tp;
  const u32 cmask = (1u << C) - 1, pmask = (1u << Tp) - 1;
  const u32 lb = strided ? C : 0;
  // tile element (q, e) -> point of plaintext p0 + q
  auto gidx = [&](u32 e) {
    e &= pmask;
    return strided ? base + ((e >> C) << a.b_lo) + (e & cmask) : base + e;
  };

  for (u32 e = threadIdx.x; e < (1u << T); e += kFftThreads) {
    const u32 g = gidx(e), p = p0 + (e >> Tp);
    double2 v = make_double2(0.0, 0.0);
    if (p < sp.count) {
      if (a.in_mode == kInCoeff) {
        const double* x = static_cast<const double*>(a.in) + (u64)p * 2 * n;
        const u32 k = brev0(g, a.ln);
        v = make_double2(x[k], x[k + n]);
      } else {
        v = static_cast<const double2*>(a.in)[(u64)p * n + g];
      }
    }
    lds[lpad(e)] = v;
  }
  __syncthreads();

  for (u32 st = 0; st < a.B; ++st) {
    const u32 i = ENC ? a.B - 1 - st : st;
    const u32 pb = lb + i;
    const u32 gb = a.b_lo + i;
    const u32 lqm = (8u << gb) - 1, wsh = sp.wbase - gb;
    for (u32 k = threadIdx.x; k < (1u << (T - 1)); k += kFftThreads) {
      const u32 ea = ((k >> pb) << (pb + 1)) | (k & ((1u << pb) - 1));
      const u32 eb = ea + (1u << pb);
      const u32 j = gidx(ea) & ((1u << gb) - 1);
      const u32 r = a.rot[j] & lqm;
      const double2 w = a.roots[(ENC ? lqm + 1 - r : r) << wsh];
      butterfly<ENC>(lds[lpad(ea)], lds[lpad(eb)], w);
    }
    __syncthreads();
  }

  if (a.out_mode == kOutRound) {
    // output rank o = (q, im, kk, r): coefficient ((im n_s + k) gap + r) of plaintext p0 + q,
    // k = (kk, bitrev(tl)) the bit reversal of the point (tl, bitrev(kk))
    const u32 lo_bits = a.ln - Tp, klo = brev0(tl, lo_bits);
    const u32 log_n = a.ln + 1 + sp.lg, per = T + 1 + sp.lg - sp.S;
    long long* c = static_cast<long long*>(a.out);
    for (u32 i = threadIdx.x; i < (1u << per); i += kFftThreads) {
      const u32 o = (sl << per) + i;
      const u32 t = o >> sp.lg, q = t >> (Tp + 1);
      if (p0 + q >= sp.count) break;  // ranks ascend in q
      const u32 kk = t & pmask, im = (t >> Tp) & 1;
      long long val = 0;
      if ((o & ((1u << sp.lg) - 1)) == 0) {
        const double2 v = lds[lpad((q << Tp) | brev0(kk, Tp))];
        val = (long long)rint((im ? v.y : v.x) * a.scale);
      }
      const u64 k = ((u64)kk << lo_bits) | klo;
      c[((u64)(p0 + q) << log_n) + ((((u64)im << a.ln) + k) << sp.lg) + (o & ((1u << sp.lg) - 1))] =
          val;
    }
    return;
  }
  for (u32 e = threadIdx.x; e < (1u << T); e += kFftThreads) {
    const u32 g = gidx(e), p = p0 + (e >> Tp);
    if (p >= sp.count) break;
    const double2 v = lds[lpad(e)];
    static_cast<double2*>(a.out)[(u64)p * n + g] =
        a.out_mode == kOutDivide ? make_double2(v.x / a.scale, v.y / a.scale) : v;
  }
}

template <bool ENC>
int launch_sparse_pass(const SparsePass& sp, hipStream_t s) {
  const u64 groups = ((u64)sp.count + (1u << sp.P) - 1) >> sp.P;
  const u64 blocks = (groups * sp.f.tiles) << sp.S;
  if (int rc = check_grid(blocks, kFftThreads, 1, 1, ENC ? "encode" : "decode")) return rc;
  k_sfft_sparse<ENC><<<dim3((u32)blocks), kFftThreads, 0, s>>>(sp);
  FHE_HIP_CHECK(hipGetLastError());
  return kOk;
}

// launch_sfft on 2^ls < N / 2 slots: ENC slots [count][n_s] -> int64 coefficients [count][N]
// (scale = delta / n_s), else doubles [count][2 n_s] -> slots (scale = delta).
template <bool ENC>
int launch_sfft_sparse(const fhe_ctx* c, const void* in, void* out, double2* work, double scale,
                       u32 ls, u32 count, hipStream_t s) {
  SparsePass sp{};
  sp.f.roots = c->d_enc_roots;
  sp.f.rot = c->d_enc_rot;
  sp.f.scale = scale;
  sp.f.ln = ls;
  sp.f.T = std::min<u32>(ls, kTileLog);
  sp.f.tiles = 1u << (ls - sp.f.T);
  sp.wbase = c->log_n - 2;
  sp.lg = c->log_n - 1 - ls;
  sp.count = count;
  SparsePass contiguous = sp;
  contiguous.f.C = sp.f.T;
  contiguous.f.b_lo = 0;
  contiguous.f.B = sp.f.T;
  // the slices of the contiguous pass's rounding store (its tile holds 2^P plaintexts)
  auto slices = [&](SparsePass& x) {
    const u32 outs = x.f.T + x.P + 1 + x.lg;
    x.S = outs > kStoreLog ? outs - kStoreLog : 0;
  };
  if (ls <= (u32)kTileLog) {
    SparsePass x = contiguous;
    u32 cl = 0;  // ceil(log2 count)
    while ((1u << cl) < count && cl < (u32)kTileLog) ++cl;
    x.P = std::min<u32>(kTileLog - ls, cl);
    if (ENC) {
      x.P = std::min<u32>(x.P, c->log_n < kStoreLog ? kStoreLog - c->log_n : 0);
      slices(x);
    }
    x.f.in = in;
    x.f.out = out;
    x.f.in_mode = ENC ? kInComplex : kInCoeff;
    x.f.out_mode = ENC ? kOutRound : kOutDivide;
    return launch_sparse_pass<ENC>(x, s);
  }
  SparsePass strided = sp;
  strided.f.B = ls - kTileLog;
  strided.f.C = kTileLog - strided.f.B;
  strided.f.b_lo = kTileLog;
  if (ENC) slices(contiguous);
  SparsePass first = ENC ? strided : contiguous, second = ENC ? contiguous : strided;
  first.f.in = in;
  first.f.out = work;
  first.f.in_mode = ENC ? kInComplex : kInCoeff;
  first.f.out_mode = kOutComplex;
  second.f.in = work;
  second.f.out = out;
  second.f.in_mode = kInComplex;
  second.f.out_mode = ENC ? kOutRound : kOutDivide;
  if (int rc = launch_sparse_pass<ENC>(first, s)) return rc;
  return launch_sparse_pass<ENC>(second, s);
}

// The unfused lift (wide contexts): coefficients [count][N] -> out [count][rows][N], canonical
// residues of every row's limb, to be NTT'd in place.  Grid y = row, z = plaintext.
__global__ __launch_bounds__(kFftThreads) void k_encode_spread(u64* __restrict__ out,
                                                               const long long* __restrict__ cf,
                                                               u32 rows, u32 level, u32 L,
                                                               u32 log_n,
                                                               const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n;
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 r = blockIdx.y;
  const u64 p = blockIdx.z;
  const ModParams m = mods[enc_limb(r, level, L)];
  out[(p * rows + r) * n + i] = lift_signed((u64)cf[p * n + i], m);
}

// Decode's centring: x [count][nl][N] = INTT of limb 0 (and limb 1 when nl == 2) -> the centred
// value over q_0 (q_0 q_1) as one round-to-nearest-even double, d [count][N].
__device__ __forceinline__ double centre_value(const u64* __restrict__ x, u64 p, u64 i, u32 nl,
                                               u64 n, ulonglong2 q0inv,
                                               const ModParams* __restrict__ mods) {
  const u64 q0 = mods[0].q;
  const u64 x0 = x[(p * nl) * n + i];
  u128 mag;
  bool neg;
  if (nl == 1) {
    neg = x0 > (q0 - 1) / 2;
    mag = neg ? q0 - x0 : x0;
  } else {
    const ModParams m1 = mods[1];
    const u64 x1 = x[(p * nl + 1) * n + i];
    const u64 a0 = reduce_word(x0, m1);
    const u64 df = x1 >= a0 ? x1 - a0 : x1 + m1.q - a0;
    const u64 t = csub(shoup_lazy(df, q0inv.x, q0inv.y, m1.q), m1.q);
    const u128 Q = (u128)q0 * m1.q;
    const u128 V = (u128)x0 + (u128)q0 * t;
    neg = V > (Q - 1) / 2;
    mag = neg ? Q - V : V;
  }
  // |V| -> double with one rounding: the top 64 bits in one word, the dropped bits' sticky OR'd
  // into bit 0 (the word's own conversion then rounds to nearest even as the 128-bit value would)
  const u64 hi = (u64)(mag >> 64);
  double v;
  if (hi == 0) {
    v = (double)(u64)mag;
  } else {
    const int sh = 64 - __clzll((long long)hi);
    u64 w = (u64)(mag >> sh);
    if ((u64)mag << (64 - sh)) w |= 1;
    v = ldexp((double)w, sh);
  }
  return neg ? -v : v;
}

__global__ __launch_bounds__(kFftThreads) void k_decode_centre(double* __restrict__ d,
                                                               const u64* __restrict__ x, u32 nl,
                                                               u32 log_n, ulonglong2 q0inv,
                                                               const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n;
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 p = blockIdx.y;
  d[p * n + i] = centre_value(x, p, i, nl, n, q0inv, mods);
}

// The same of the coefficients k gap only (sparse packing): d [count][2 n_s], 2 n_s = N >> lg.
__global__ __launch_bounds__(kFftThreads) void k_decode_centre_sparse(
    double* __restrict__ d, const u64* __restrict__ x, u32 nl, u32 log_n, u32 lg,
    ulonglong2 q0inv, const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n, m = n >> lg;
  const u64 k = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const u64 p = blockIdx.y;
  if (k < m) d[p * m + k] = centre_value(x, p, k << lg, nl, n, q0inv, mods);
}

}  // namespace

size_t encode_workspace_bytes(const fhe_ctx* c, u32 count) {
  // the FFT's workspace [count][n] complex, then the coefficients [count][N]
  return (size_t)2 * count * c->n * sizeof(u64);
}

size_t decode_workspace_bytes(const fhe_ctx* c, u32 count) {
  // INTT of limbs 0, 1 [count][2][N] (the FFT's workspace afterwards), then the doubles [count][N]
  return (size_t)3 * count * c->n * sizeof(u64);
}

int launch_encode_coeffs(const fhe_ctx* c, long long* cf, const double* slots, double delta,
                         u32 log_slots, u32 count, void* work, hipStream_t s) {
  if (count == 0) return kOk;
  const bool full = log_slots == c->log_n - 1;
  const double scale = delta / (double)(1ull << log_slots);
  double2* w = static_cast<double2*>(work);
  if (int rc = full ? launch_sfft<true>(c, slots, cf, w, scale, count, s)
                    : launch_sfft_sparse<true>(c, slots, cf, w, scale, log_slots, count, s))
    return rc;
  prof_mark(s, "encode_fft");
  return kOk;
}

int launch_encode_spread(const fhe_ctx* c, u64* out, const long long* cf, u32 rows, u32 level,
                         u32 count, hipStream_t s) {
  if ((u64)count * rows == 0) return kOk;
  if (int rc = check_grid(c->n / kFftThreads, kFftThreads, rows, count, "encode")) return rc;
  k_encode_spread<<<dim3((u32)(c->n / kFftThreads), rows, count), kFftThreads, 0, s>>>(
      out, cf, rows, level, c->L, c->log_n, c->d_mods);
  FHE_HIP_CHECK(hipGetLastError());
  return kOk;
}

int launch_encode(const fhe_ctx* c, u64* out, const double* slots, double delta, u32 log_slots,
                  u32 level, bool special, u32 count, void* ws, bool unfused, hipStream_t s) {
  if (count == 0) return kOk;
  const u64 n = c->n;
  const u32 rows = level + (special ? c->K : 0);
  long long* cf = reinterpret_cast<long long*>(static_cast<u64*>(ws) + (u64)count * n);
  int rc;
  if ((rc = launch_encode_coeffs(c, cf, slots, delta, log_slots, count, ws, s))) return rc;
  const u64 ps = (u64)rows * n;
  if (!c->wide && !unfused) {
    // the lift rides on the column-forward pass (ntt.hip k_lift_col); the row pass runs in place
    if ((rc = launch_encode_col(c, reinterpret_cast<const u64*>(cf), out, count, level, rows, s)))
      return rc;
    if ((rc = launch_ntt_row_fwd_r2(c, out, ps, out, ps, count, 0, level, s))) return rc;
    if (special &&
        (rc = launch_ntt_row_fwd_r2(c, out + (u64)level * n, ps, out + (u64)level * n, ps, count,
                                    c->L, c->K, s)))
      return rc;
  } else {
    if ((rc = launch_encode_spread(c, out, cf, rows, level, count, s))) return rc;
    if ((rc = launch_ntt(c, true, out, out, count, ps, 0, level, s))) return rc;
    if (special && (rc = launch_ntt(c, true, out + (u64)level * n, out + (u64)level * n, count, ps,
                                    c->L, c->K, s)))
      return rc;
  }
  prof_mark(s, "encode_ntt");
  return kOk;
}

namespace {
// What fhe_decode and fhe_decrypt_slots share: x = ws [count][nl][N] holds the inverse transforms
// of limb 0 (and 1); centring into the doubles behind it, then the special FFT into slots.
int decode_tail(const fhe_ctx* c, double* slots, double delta, u32 log_slots, u32 nl, u32 count,
                void* ws, hipStream_t s) {
  const u64 n = c->n;
  u64* x = static_cast<u64*>(ws);
  double* d = reinterpret_cast<double*>(x + (u64)2 * count * n);
  int rc;
  const bool full = log_slots == c->log_n - 1;
  if (full) {
    if ((rc = check_grid(n / kFftThreads, kFftThreads, count, 1, "decode"))) return rc;
    k_decode_centre<<<dim3((u32)(n / kFftThreads), count), kFftThreads, 0, s>>>(
        d, x, nl, c->log_n, c->enc_q0inv, c->d_mods);
  } else {
    const u32 lg = c->log_n - 1 - log_slots;
    const u32 bx = (u32)(((n >> lg) + kFftThreads - 1) / kFftThreads);
    if ((rc = check_grid(bx, kFftThreads, count, 1, "decode"))) return rc;
    k_decode_centre_sparse<<<dim3(bx, count), kFftThreads, 0, s>>>(d, x, nl, c->log_n, lg,
                                                                    c->enc_q0inv, c->d_mods);
  }
  FHE_HIP_CHECK(hipGetLastError());
  prof_mark(s, "decode_centre");
  // x is dead: its region is the FFT's workspace
  double2* work = reinterpret_cast<double2*>(x);
  if ((rc = full ? launch_sfft<false>(c, d, slots, work, delta, count, s)
                 : launch_sfft_sparse<false>(c, d, slots, work, delta, log_slots, count, s)))
    return rc;
  prof_mark(s, "decode_fft");
  return kOk;
}
}  // namespace

int launch_decode(const fhe_ctx* c, double* slots, const u64* pt, double delta, u32 log_slots,
                  u32 pt_rows, u32 level, u32 count, void* ws, hipStream_t s) {
  if (count == 0) return kOk;
  const u64 n = c->n;
  const u32 nl = level >= 2 ? 2 : 1;
  u64* x = static_cast<u64*>(ws);  // [count][nl][N]
  if (int rc = launch_ntt_strided(c, false, pt, (u64)pt_rows * n, x, (u64)nl * n, count, 0, nl, s))
    return rc;
  prof_mark(s, "decode_intt");
  return decode_tail(c, slots, delta, log_slots, nl, count, ws, s);
}

int launch_decrypt_slots(const fhe_ctx* c, double* slots, const u64* ct, const u64* sk,
                         double delta, u32 log_slots, u32 level, u32 batch, void* ws, bool unfused,
                         hipStream_t s) {
  if (batch == 0) return kOk;
  const u64 n = c->n;
  const u32 nl = level >= 2 ? 2 : 1;
  u64* x = static_cast<u64*>(ws);  // [batch][nl][N]: c0 + c1 s, inverse-transformed in place
  int rc;
  if (!c->wide && !unfused) {
    // the product rides on the inverse transform's first pass (ntt.hip k_dec_row)
    if ((rc = launch_dec_row(c, ct, sk, x, level, nl, batch, s))) return rc;
    prof_mark(s, "decrypt_row");
    if ((rc = launch_ntt_col_inv(c, x, (u64)nl * n, x, (u64)nl * n, batch, 0, nl, s, nullptr,
                                 false, "decode_col_inv")))
      return rc;
  } else {
    if ((rc = launch_decrypt_rows(c, x, ct, sk, level, nl, batch, s))) return rc;
    prof_mark(s, "decrypt_mac");
    if ((rc = launch_ntt(c, false, x, x, batch, (u64)nl * n, 0, nl, s))) return rc;
    prof_mark(s, "decode_intt");
  }
  return decode_tail(c, slots, delta, log_slots, nl, batch, ws, s);
}

}  // namespace fhe
