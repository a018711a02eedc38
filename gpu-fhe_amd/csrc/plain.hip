// Level-aware plaintext arithmetic on NTT-form ciphertexts (fhe_lincomb_level, fhe_mul_plain_level;
// include/fhecore.h): out = [rescale]( sum_i k_i cts[i]|_level (+ k_count on c0) ) with per-limb
// scalar residues, and out = [rescale]( ct * pt ) with a per-element plaintext row.
//
// One kernel body, k_lincomb: one poly-limb row of the OUTPUT per blockIdx.y (its ModParams and
// its scalars uniform: scalar loads), a 16-byte pair per lane, non-temporal loads and stores as
// k_vec_ctx (elementwise.hip) -- every operand word is touched once.  Term t of polynomial p, limb
// l starts at src[t] + p pstride[t] + l N with pstride[t] = in_levels[t] N: a term at a higher
// level is cut to `level` limbs through its own stride (the level drop costs no pass).  All terms
// are read in the one pass, kTermGroup loads in flight per lane; 8 (count + 1) bytes per element.
//
// Accumulation (LcMode):
//  * kLcNarrow (every context modulus < 2^61): the products k_i x_i < 2^122 and the constant sum
//    in 128 bits (16 terms + constant < 2^126 + 2^61) and reduce once with reduce128 -- one
//    reduction per element whatever the count;
//  * kLcWide (some modulus in [2^61, 2^63)): each product reduced to [0, q) by barrett_reduce
//    (reduce128_wide for a wide limb) and added with one conditional subtraction (a + b < 2q < 2^64);
//  * kLcRows (fhe_mul_plain_level): the one term's multiplier is the plaintext's element, the
//    product reduced as fhe_vec_mul reduces it (mulmod_barrett).
// Every form returns the canonical residue.
#include "internal.hpp"

namespace fhe {
namespace {

constexpr int kLcThreads = 128;  // k_vec_ctx's workgroup: 2 waves, one pair per lane
constexpr u32 kTermGroup = 4;    // loads issued before the first product of a group
typedef u64 vu64x2 __attribute__((ext_vector_type(2)));

enum LcMode : int { kLcNarrow = 0, kLcWide = 1, kLcRows = 2 };

struct LincombArgs {
  const u64* src[kLincombMax];
  u64 pstride[kLincombMax];  // words between polynomials of term t: in_levels[t] * N
  const u64* scalars;        // [count + 1][sstride] residues (kLcRows: unused)
  const u64* rows;           // kLcRows: plaintext, row l of ciphertext b at rows + b rows_bs + l N
  u64 rows_bs;               // 0: one plaintext for the whole batch
  u32 sstride, count, has_const, level, row_pairs, nrows;
};

template <int MODE>
__global__ __launch_bounds__(kLcThreads) void k_lincomb(u64* out, const LincombArgs a,
                                                       const ModParams* __restrict__ mods) {
  const u32 i = blockIdx.x * kLcThreads + threadIdx.x;
  if (i >= a.row_pairs) return;
  for (u32 row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    const u32 poly = row / a.level, l = row - poly * a.level;
    const ModParams m = mods[l];
    const u64 roff = (u64)l * a.row_pairs;  // in pairs
    vu64x2 r;
    if constexpr (MODE == kLcRows) {
      const vu64x2 x = __builtin_nontemporal_load(
          reinterpret_cast<const vu64x2*>(a.src[0] + poly * a.pstride[0]) + roff + i);
      // the plaintext row serves both polynomials of a ciphertext (and every ciphertext when
      // rows_bs == 0): a cached load
      const vu64x2 y =
          (reinterpret_cast<const vu64x2*>(a.rows + (u64)(poly >> 1) * a.rows_bs) + roff)[i];
      r = vu64x2{mulmod_barrett(x.x, y.x, m), mulmod_barrett(x.y, y.y, m)};
    } else {
      // the constant polynomial k is k at every NTT slot: added to c0 (even polys) only
      const u64 k0 = (a.has_const && !(poly & 1)) ? a.scalars[(u64)a.count * a.sstride + l] : 0;
      u128 s0 = k0, s1 = k0;  // kLcNarrow
      u64 w0 = k0, w1 = k0;   // kLcWide
      for (u32 t0 = 0; t0 < a.count; t0 += kTermGroup) {
        vu64x2 x[kTermGroup];
        u64 k[kTermGroup];
#pragma unroll
        for (u32 u = 0; u < kTermGroup; ++u) {
          const u32 t = t0 + u;
          if (t < a.count) {
            x[u] = __builtin_nontemporal_load(
                reinterpret_cast<const vu64x2*>(a.src[t] + poly * a.pstride[t]) + roff + i);
            k[u] = a.scalars[(u64)t * a.sstride + l];
          }
        }
#pragma unroll
        for (u32 u = 0; u < kTermGroup; ++u) {
          if (t0 + u < a.count) {
            if constexpr (MODE == kLcNarrow) {
              s0 += (u128)x[u].x * k[u];
              s1 += (u128)x[u].y * k[u];
            } else {
              w0 = csub(w0 + mulmod_barrett(x[u].x, k[u], m), m.q);
              w1 = csub(w1 + mulmod_barrett(x[u].y, k[u], m), m.q);
            }
          }
        }
      }
      if constexpr (MODE == kLcNarrow)
        r = vu64x2{reduce128((u64)s0, (u64)(s0 >> 64), m), reduce128((u64)s1, (u64)(s1 >> 64), m)};
      else
        r = vu64x2{w0, w1};
    }
    __builtin_nontemporal_store(r, reinterpret_cast<vu64x2*>(out) + (u64)row * a.row_pairs + i);
  }
}

int launch(const fhe_ctx* c, int mode, u64* out, LincombArgs& a, u32 batch, u32 level,
           const char* who, hipStream_t s) {
  const u64 rows64 = (u64)batch * 2 * level;
  if (rows64 == 0) return kOk;
  if (rows64 > 0xffffffffull) {
    set_error(std::string(who) + ": too many poly-limb rows");
    return kInvalid;
  }
  a.level = level;
  a.nrows = (u32)rows64;
  a.row_pairs = (u32)(c->n / 2);  // N >= 2^10: whole pairs per row
  const dim3 g((a.row_pairs + kLcThreads - 1) / kLcThreads, a.nrows < 65535 ? a.nrows : 65535);
  switch (mode) {
    case kLcNarrow: k_lincomb<kLcNarrow><<<g, kLcThreads, 0, s>>>(out, a, c->d_mods); break;
    case kLcWide: k_lincomb<kLcWide><<<g, kLcThreads, 0, s>>>(out, a, c->d_mods); break;
    default: k_lincomb<kLcRows><<<g, kLcThreads, 0, s>>>(out, a, c->d_mods); break;
  }
  FHE_HIP_CHECK(hipGetLastError());
  prof_mark(s, mode == kLcRows ? "mul_plain" : "lincomb");
  return kOk;
}

// the sum lands in the workspace's first batch * 2 * level * N words, the rescale's own regions
// behind the batch * 2 * L * N reserved for it
int finish(const fhe_ctx* c, int mode, u64* out, LincombArgs& a, u32 batch, u32 level,
           bool rescale, void* ws, const char* who, hipStream_t s) {
  if (!rescale) return launch(c, mode, out, a, batch, level, who, s);
  u64* sum = static_cast<u64*>(ws);
  if (int rc = launch(c, mode, sum, a, batch, level, who, s)) return rc;
  return launch_rescale(c, out, sum, 2 * batch, level, true, sum + (u64)batch * 2 * c->L * c->n, s);
}

// conj_split / conj_merge (fhe_conj_split_level / fhe_conj_merge_level).  X^(N/2) multiplies every
// slot by i and is, in NTT layout, the constant w_l = psi_l^(N/2) at elements k < N/2 of limb l
// and q_l - w_l at k >= N/2 (element k evaluates at psi^(2 brv(k) + 1), and brv(k) is odd exactly
// when the top bit of k is set), so the side is uniform over a workgroup's pairs.
//   split: re = x + y, im = -X^(N/2) (x - y) = w (y - x) | w (x - y)   (first | second half)
//   merge: re = x + X^(N/2) y              = x + w y   | x - w y
// The product by w is the exact-quotient Shoup form, [0, 2q) with 2q < 2^64 for every context
// modulus (wide ones included), then one conditional subtraction: canonical in and out.  The
// pointers may alias element for element (an output that is an input), so none is __restrict__
// and every element is read before it is written by the one lane that owns it.
template <bool MERGE>
__global__ __launch_bounds__(kLcThreads) void k_conj(u64* re, u64* im, const u64* x, const u64* y,
                                                    u32 level, u32 row_pairs, u32 nrows,
                                                    const ulonglong2* __restrict__ wtab,
                                                    const ModParams* __restrict__ mods) {
  const u32 i = blockIdx.x * kLcThreads + threadIdx.x;
  if (i >= row_pairs) return;
  const bool second = i >= row_pairs / 2;
  for (u32 row = blockIdx.y; row < nrows; row += gridDim.y) {
    const u32 l = row % level;
    const u64 q = mods[l].q;
    const ulonglong2 w = wtab[l];
    const u64 at = (u64)row * row_pairs + i;
    const vu64x2 a = __builtin_nontemporal_load(reinterpret_cast<const vu64x2*>(x) + at);
    const vu64x2 b = __builtin_nontemporal_load(reinterpret_cast<const vu64x2*>(y) + at);
    vu64x2 r0, r1;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const u64 u = e ? a.y : a.x, v = e ? b.y : b.x;
      u64 o0, o1 = 0;
      if constexpr (MERGE) {
        const u64 t = csub(shoup_lazy(v, w.x, w.y, q), q);
        o0 = second ? (u >= t ? u - t : u + (q - t)) : csub(u + t, q);
      } else {
        o0 = csub(u + v, q);
        const u64 d = second ? (u >= v ? u - v : u + (q - v)) : (v >= u ? v - u : v + (q - u));
        o1 = csub(shoup_lazy(d, w.x, w.y, q), q);
      }
      if (e) r0.y = o0, r1.y = o1; else r0.x = o0, r1.x = o1;
    }
    __builtin_nontemporal_store(r0, reinterpret_cast<vu64x2*>(re) + at);
    if constexpr (!MERGE) __builtin_nontemporal_store(r1, reinterpret_cast<vu64x2*>(im) + at);
  }
}

}  // namespace

int launch_conj(const fhe_ctx* c, bool merge, u64* re, u64* im, const u64* ct, const u64* cc,
                u32 level, u32 batch, hipStream_t s) {
  const u64 rows64 = (u64)batch * 2 * level;
  if (rows64 == 0) return kOk;
  if (rows64 > 0xffffffffull) {
    set_error("conj_split / conj_merge: too many poly-limb rows");
    return kInvalid;
  }
  const u32 nrows = (u32)rows64, row_pairs = (u32)(c->n / 2);  // N >= 2^10: whole pairs per row
  const dim3 g((row_pairs + kLcThreads - 1) / kLcThreads, nrows < 65535 ? nrows : 65535);
  if (merge)
    k_conj<true><<<g, kLcThreads, 0, s>>>(re, im, ct, cc, level, row_pairs, nrows, c->d_conj_w, c->d_mods);
  else
    k_conj<false><<<g, kLcThreads, 0, s>>>(re, im, ct, cc, level, row_pairs, nrows, c->d_conj_w, c->d_mods);
  FHE_HIP_CHECK(hipGetLastError());
  prof_mark(s, merge ? "conj_merge" : "conj_split");
  return kOk;
}

size_t lincomb_workspace_bytes(const fhe_ctx* c, u32 batch) {
  return (size_t)batch * 2 * c->L * c->n * sizeof(u64) + rescale_workspace_bytes(c, 2 * batch, c->L);
}

int launch_lincomb(const fhe_ctx* c, u64* out, const u64* const* cts, const u32* in_levels,
                   const u64* scalars, u32 scalar_stride, bool has_const, u32 level, u32 count,
                   u32 batch, bool rescale, void* ws, hipStream_t s) {
  LincombArgs a{};
  for (u32 t = 0; t < count; ++t) {
    a.src[t] = cts[t];
    a.pstride[t] = (u64)in_levels[t] * c->n;
  }
  a.scalars = scalars;
  a.sstride = scalar_stride;
  a.count = count;
  a.has_const = has_const ? 1 : 0;
  return finish(c, c->wide ? kLcWide : kLcNarrow, out, a, batch, level, rescale, ws, "lincomb", s);
}

int launch_mul_plain(const fhe_ctx* c, u64* out, const u64* ct, const u64* pt, u32 pt_rows,
                     u32 pt_batch, u32 level, u32 batch, bool rescale, void* ws, hipStream_t s) {
  LincombArgs a{};
  a.src[0] = ct;
  a.pstride[0] = (u64)level * c->n;
  a.count = 1;
  a.rows = pt;
  a.rows_bs = pt_batch == 1 ? 0 : (u64)pt_rows * c->n;
  return finish(c, kLcRows, out, a, batch, level, rescale, ws, "mul_plain", s);
}

}  // namespace fhe
