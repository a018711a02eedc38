// Sampling, key generation, encryption and decryption: the operations
// that turn HomMult / key-switch / rotation into end-to-end checks with real keys.  Not in the
// reference; restated by oracle/pyoracle.py (philox, sample_*, keygen_*, encrypt_*, decrypt).
//
// Randomness is counter-based (Philox4x32-10, the Random123 construction), so every sample is a
// pure function of (seed, stream tag, poly, limb, coefficient): GPU and oracle agree bit for bit
// and no generator state lives on the device.
//   uniform mod q   floor(r q / 2^128) of a 128-bit draw (bias < 2^-67 for q < 2^61)
//   ternary         (r mod 3) - 1 of a 32-bit draw, the same integer on every limb
//   sparse ternary  exactly h coefficients +-1: the h smallest 64-bit keys (r.x << 32) | c
//                   (fhe_keygen_secret_sparse; restated by oracle/pyoracle.py)
//   error           centred binomial, eta = 21 (sd ~3.2): popcount of 21 bits minus 21 bits
// Keys and ciphertexts are NTT form over their limbs (the layout of the rest of the library).
#include "../../include/fhecore.h"
#include "internal.hpp"

namespace fhe {
namespace {

constexpr int kThreads = 256;

struct P4 {
  u32 x, y, z, w;
};

__host__ __device__ inline P4 philox4x32_10(P4 c, u32 k0, u32 k1) {
  constexpr u32 M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)M0 * c.x, p1 = (u64)M1 * c.z;
    c = P4{(u32)(p1 >> 32) ^ c.y ^ k0, (u32)p1, (u32)(p0 >> 32) ^ c.w ^ k1, (u32)p0};
    k0 += W0;
    k1 += W1;
  }
  return c;
}

enum Kind : int { kUniform = 0, kTernary = 1, kError = 2 };

// The draws, one definition each: (coefficient c, poly p, stream tag) under the key (k0, k1).
// uniform mod q takes the limb's own index into the counter; a small draw is limb-free.
__device__ __forceinline__ u64 draw_uniform(u32 c, u32 limb, u32 p, u32 tag, u32 k0, u32 k1, u64 q) {
  const P4 r = philox4x32_10(P4{c, limb, p, tag}, k0, k1);
  const u64 lo = ((u64)r.y << 32) | r.x, hi = ((u64)r.w << 32) | r.z;
  const u128 t = (u128)hi * q + (u64)(((u128)lo * q) >> 64);
  return (u64)(t >> 64);
}

__device__ __forceinline__ int64_t draw_small(int kind, u32 c, u32 p, u32 tag, u32 k0, u32 k1) {
  const P4 r = philox4x32_10(P4{c, 0xffffffffu, p, tag}, k0, k1);
  if (kind == kTernary) return (int64_t)(r.x % 3u) - 1;
  const u64 bits = ((u64)r.y << 32) | r.x;
  return (int64_t)__popcll(bits & 0x1fffffull) - (int64_t)__popcll((bits >> 21) & 0x1fffffull);
}

// out rows [poly][limb][N] (poly stride pstride) over ctx limbs limb0 + l.  Grid: x over
// coefficients, y = limb, z = poly.  The draw for (poly, coefficient) of a small distribution does
// not depend on the limb, so every limb holds the same integer.
__global__ __launch_bounds__(kThreads) void k_sample(u64* __restrict__ out, u64 pstride,
                                                     u32 limb0, u32 log_n, int kind, u32 seed_lo,
                                                     u32 seed_hi, u32 tag,
                                                     const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 l = blockIdx.y, p = blockIdx.z;
  const u32 limb = limb0 + l;
  const u64 q = mods[limb].q;
  u64 v;
  if (kind == kUniform) {
    v = draw_uniform(c, limb, p, tag, seed_lo, seed_hi, q);
  } else {
    const int64_t s = draw_small(kind, c, p, tag, seed_lo, seed_hi);
    v = s >= 0 ? (u64)s : q - (u64)(-s);
  }
  out[(u64)p * pstride + (u64)l * n + c] = v;
}

// out = x + y * s over [polys][nlimbs][N] rows, NTT form: c0 + c1 s (decryption) and friends.
// s has one row per limb (broadcast over polys).  Grid: x over coefficients, y = limb, z = poly.
__global__ __launch_bounds__(kThreads) void k_mac_s(u64* __restrict__ out, u64 pout,
                                                    const u64* __restrict__ x, u64 px,
                                                    const u64* __restrict__ y, u64 py,
                                                    const u64* __restrict__ s, u32 limb0,
                                                    u32 log_n, int negate,
                                                    const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 l = blockIdx.y;
  const u64 p = blockIdx.z;
  const ModParams m = mods[limb0 + l];
  const u64 off = (u64)l * n + c;
  u64 t = mulmod_barrett(y[p * py + off], s[off], m);
  if (negate) t = t ? m.q - t : 0;
  out[p * pout + off] = csub((x ? x[p * px + off] : 0) + t, m.q);
}

// row[c] = (row[c] + k y[c]) mod q for one limb; k a constant with its Shoup companion.
__global__ __launch_bounds__(kThreads) void k_axpy_const(u64* __restrict__ row,
                                                         const u64* __restrict__ y, u64 k, u64 ks,
                                                         u64 q) {
  const u64 c = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  row[c] = csub(row[c] + csub(shoup_lazy(y[c], k, ks, q), q), q);
}

int sample(const fhe_ctx* c, u64* out, u64 pstride, u32 polys, u32 limb0, u32 nlimbs, int kind,
           u64 seed, u32 tag, hipStream_t s) {
  if ((u64)polys * nlimbs == 0) return kOk;
  if (int rc = check_grid(c->n / kThreads, kThreads, nlimbs, polys, "sample")) return rc;
  k_sample<<<dim3((u32)(c->n / kThreads), nlimbs, polys), kThreads, 0, s>>>(
      out, pstride, limb0, c->log_n, kind, (u32)seed, (u32)(seed >> 32), tag, c->d_mods);
  FHE_HIP_CHECK(hipGetLastError());
  return kOk;
}

int mac_s(const fhe_ctx* c, u64* out, u64 pout, const u64* x, u64 px, const u64* y, u64 py,
          const u64* sk, u32 polys, u32 limb0, u32 nlimbs, bool negate, hipStream_t s) {
  if ((u64)polys * nlimbs == 0) return kOk;
  if (int rc = check_grid(c->n / kThreads, kThreads, nlimbs, polys, "mac_s")) return rc;
  k_mac_s<<<dim3((u32)(c->n / kThreads), nlimbs, polys), kThreads, 0, s>>>(
      out, pout, x, px, y, py, sk, limb0, c->log_n, negate ? 1 : 0, c->d_mods);
  FHE_HIP_CHECK(hipGetLastError());
  return kOk;
}

// stream tags: which draw a sample belongs to (same seed, disjoint counters)
enum Tag : u32 { kTagSecret = 1, kTagPkA = 2, kTagPkE = 3, kTagSparse = 4, kTagKsA = 0x100,
                 kTagKsE = 0x101, kTagEncU = 32, kTagEncE0 = 33, kTagEncE1 = 34, kTagEncA = 35,
                 kTagEncE = 36 };

// ---- batched encryption at any level (fhe_encrypt_level / _sk_level / _slots) -------------------
// Ciphertext b of a pass is poly j = poly0 + b of the Philox counter.  Three steps:
//   k_enc_draw    one Philox draw per (ciphertext, polynomial, coefficient), written as the signed
//                 word the encoder's lift takes; the message's coefficients (fhe_encrypt_slots)
//                 are added to e0 / e here, since the NTT is linear
//   lift + NTT    launch_encode_col + launch_ntt_row_fwd_r2 (ntt.hip), or on wide contexts a spread
//                 and whole NTTs: e0, e1 straight into ct, u (or the secret-key form's e) into
//                 the workspace
//   k_enc_finish  one pass over ct: in place + b u^ + pt, + a u^ (public key), or a drawn inline
//                 as c1 and c0 = e^ - a s + pt (secret key)
// Both kernels are shaped like k_lincomb (plain.hip): a row per blockIdx.y (its draw kind, tag,
// ModParams uniform), a 16-byte pair per lane, rows beyond the grid's y limit by stride.
constexpr int kEncThreads = 128;
typedef u64 vu64x2 __attribute__((ext_vector_type(2)));
typedef long long vi64x2 __attribute__((ext_vector_type(2)));

struct EncDraw {
  long long* u;          // [batch][N]      public-key form only
  long long* e;          // [batch][nd - 1][N] (e0, e1), or [batch][N] (e) when nd == 1
  const long long* msg;  // [batch][N] added into e0 / e, or null
  u32 nd;                // draws per ciphertext: 3 (u, e0, e1) or 1 (e)
  u32 batch, row_pairs, poly0, seed_lo, seed_hi;
};

__global__ __launch_bounds__(kEncThreads) void k_enc_draw(const EncDraw a) {
  const u32 i = blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= a.row_pairs) return;
  const bool pkf = a.nd == 3;
  const u32 nrows = a.nd * a.batch;
  for (u32 row = blockIdx.y; row < nrows; row += gridDim.y) {
    const u32 b = row / a.nd, k = row - b * a.nd;
    const bool is_u = pkf && k == 0;
    const int kind = is_u ? kTernary : kError;
    const u32 tag = pkf ? kTagEncU + k : kTagEncE;
    long long* dst = is_u ? a.u + (u64)b * 2 * a.row_pairs
                          : a.e + ((u64)b * (pkf ? 2 : 1) + (pkf ? k - 1 : 0)) * 2 * a.row_pairs;
    vi64x2 r{draw_small(kind, 2 * i, a.poly0 + b, tag, a.seed_lo, a.seed_hi),
             draw_small(kind, 2 * i + 1, a.poly0 + b, tag, a.seed_lo, a.seed_hi)};
    if (a.msg && k == (pkf ? 1u : 0u))
      r += __builtin_nontemporal_load(reinterpret_cast<const vi64x2*>(a.msg) +
                                      (u64)b * a.row_pairs + i);
    reinterpret_cast<vi64x2*>(dst)[i] = r;  // read back by the lift: a cached store
  }
}

struct EncFinish {
  u64* ct;          // [batch][2][level][N]; public-key form: NTT(e0), NTT(e1) on entry
  const u64* that;  // [batch][level][N]: NTT(u), or NTT(e) of the secret-key form (ct has a row of
                    // e per two rows of output, so that form's transform runs beside it)
  const u64* key0;  // pk[0] = b rows, or the secret's rows     (row l at key0 + l N)
  const u64* key1;  // pk[1] = a rows                           (public-key form)
  const u64* pt;    // row l of ciphertext b at pt + b pt_bs + l N, or null
  u64 pt_bs;        // 0: one plaintext for the whole batch
  u32 level, nrows, row_pairs, poly0, seed_lo, seed_hi;
};

template <bool SK>
__global__ __launch_bounds__(kEncThreads) void k_enc_finish(const EncFinish a,
                                                           const ModParams* __restrict__ mods) {
  const u32 i = blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= a.row_pairs) return;
  for (u32 row = blockIdx.y; row < a.nrows; row += gridDim.y) {
    const u32 b = row / a.level, l = row - b * a.level;
    const ModParams m = mods[l];
    const u64 roff = (u64)l * a.row_pairs + i;  // in pairs
    vu64x2* c0 = reinterpret_cast<vu64x2*>(a.ct) + (u64)b * 2 * a.level * a.row_pairs + roff;
    vu64x2* c1 = c0 + (u64)a.level * a.row_pairs;
    vu64x2 p{0, 0};
    if (a.pt) p = (reinterpret_cast<const vu64x2*>(a.pt + (u64)b * a.pt_bs) + roff)[0];
    // the key rows serve every ciphertext: cached loads
    const vu64x2 k0 = (reinterpret_cast<const vu64x2*>(a.key0) + roff)[0];
    const vu64x2 t = __builtin_nontemporal_load(reinterpret_cast<const vu64x2*>(a.that) +
                                                (u64)b * a.level * a.row_pairs + roff);
    vu64x2 r0, r1;
    if constexpr (SK) {
      const vu64x2 e0 = t;
      r1 = vu64x2{draw_uniform(2 * i, l, a.poly0 + b, kTagEncA, a.seed_lo, a.seed_hi, m.q),
                  draw_uniform(2 * i + 1, l, a.poly0 + b, kTagEncA, a.seed_lo, a.seed_hi, m.q)};
      const u64 t0 = mulmod_barrett(r1.x, k0.x, m), t1 = mulmod_barrett(r1.y, k0.y, m);
      r0 = vu64x2{csub(e0.x + (t0 ? m.q - t0 : 0), m.q), csub(e0.y + (t1 ? m.q - t1 : 0), m.q)};
    } else {
      const vu64x2 k1 = (reinterpret_cast<const vu64x2*>(a.key1) + roff)[0];
      const vu64x2 e0 = __builtin_nontemporal_load(c0), e1 = __builtin_nontemporal_load(c1);
      const vu64x2 u = t;
      r0 = vu64x2{csub(e0.x + mulmod_barrett(k0.x, u.x, m), m.q),
                  csub(e0.y + mulmod_barrett(k0.y, u.y, m), m.q)};
      r1 = vu64x2{csub(e1.x + mulmod_barrett(k1.x, u.x, m), m.q),
                  csub(e1.y + mulmod_barrett(k1.y, u.y, m), m.q)};
    }
    r0 = vu64x2{csub(r0.x + p.x, m.q), csub(r0.y + p.y, m.q)};
    __builtin_nontemporal_store(r0, c0);
    __builtin_nontemporal_store(r1, c1);
  }
}

// ---- fixed-Hamming-weight secret (fhe_keygen_secret_sparse) --------------------------------------
// Coefficient c draws r = philox(c, 0xffffffff, 0, kTagSparse) and carries the 64-bit key
// (r.x << 32) | c: distinct keys, so "the h smallest keys" is one set whatever the order of
// evaluation.  One workgroup finds the h-th smallest key T by a radix select, 8 bits a pass from
// the top: a pass histograms the digit of every key that matches the prefix found so far (the
// draw is regenerated, nothing is stored), then every lane walks the 256 counts to the digit that
// holds rank h.  N <= 2^17: 8 passes of at most 128 draws per lane.  Coefficient c is then
// nonzero iff key_c <= T, +1 if (r.y & 1) == 0, else -1; the integer goes to `row` (the LAST limb's
// row, as a residue of q_last), which k_sparse_spread reads and never writes.
constexpr int kSelThreads = 1024;

__device__ __forceinline__ u64 sparse_key(u32 c, u32 seed_lo, u32 seed_hi, u32* sign) {
  const P4 r = philox4x32_10(P4{c, 0xffffffffu, 0, kTagSparse}, seed_lo, seed_hi);
  *sign = r.y & 1;
  return ((u64)r.x << 32) | c;
}

__global__ __launch_bounds__(kSelThreads) void k_sparse_select(u64* __restrict__ row, u32 n, u32 h,
                                                              u32 seed_lo, u32 seed_hi,
                                                              u64 q_last) {
  __shared__ u32 hist[256];
  u64 prefix = 0, mask = 0;
  u32 rank = h;  // 1-based rank of T among the keys matching (prefix, mask)
  u32 sign;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    for (u32 c = threadIdx.x; c < n; c += kSelThreads) {
      const u64 key = sparse_key(c, seed_lo, seed_hi, &sign);
      if ((key & mask) == prefix) atomicAdd(&hist[(u32)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    u32 d = 0, below = 0;  // every lane walks the same counts: no broadcast needed
    while (d < 255 && below + hist[d] < rank) below += hist[d++];
    rank -= below;
    prefix |= (u64)d << shift;
    mask |= 255ull << shift;
    __syncthreads();  // the next pass clears hist
  }
  for (u32 c = threadIdx.x; c < n; c += kSelThreads) {
    const u64 key = sparse_key(c, seed_lo, seed_hi, &sign);
    row[c] = key <= prefix ? (sign ? q_last - 1 : 1) : 0;
  }
}

// rows 0 .. nlimbs-1 of sk [nlimbs + 1][N] from the last row's integer (0, 1 or q_last - 1).
// Grid: x over coefficients, y = limb.
__global__ __launch_bounds__(kThreads) void k_sparse_spread(u64* __restrict__ sk, u32 log_n,
                                                            u32 nlimbs,
                                                            const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 l = blockIdx.y;
  const u64 v = sk[(u64)nlimbs * n + c];
  sk[(u64)l * n + c] = v <= 1 ? v : mods[l].q - 1;
}

}  // namespace

// fhe_decrypt's product on the limbs l < nl only, into x [batch][nl][N] (fhe_decrypt_slots'
// unfused form: the decoder reads no other limb)
int launch_decrypt_rows(const fhe_ctx* c, u64* x, const u64* ct, const u64* sk, u32 level, u32 nl,
                        u32 batch, hipStream_t s) {
  const u64 ln = (u64)level * c->n;
  return mac_s(c, x, (u64)nl * c->n, ct, 2 * ln, ct + ln, 2 * ln, sk, batch, 0, nl, false, s);
}

// The workspace of one pass of b ciphertexts, in words (a null base measures):
//   draws  [3 b N]          u [b][N] then (e0, e1) [b][2][N]; the secret-key form uses e [b][N].
//                           The encoder's FFT workspace [b][N/2] complex lives here first
//                           (fhe_encrypt_slots): it is dead once the coefficients are written
//   cf     [b N]            the message's coefficients (fhe_encrypt_slots)
//   that   [b level N]      NTT(u), or NTT(e) of the secret-key form
// One size serves the three calls: (4 + level) b N words.
namespace {
struct EncWs {
  u64 *draws, *cf, *that;
  u64 words;
};
EncWs enc_ws(const fhe_ctx* c, u64* base, u32 level, u32 b) {
  WsCarve w{base};
  EncWs r{};
  r.draws = w.take((u64)3 * b * c->n);
  r.cf = w.take((u64)b * c->n);
  r.that = w.take((u64)b * level * c->n);
  r.words = w.words;
  return r;
}
}  // namespace

u32 encrypt_pass_batch(const fhe_ctx* c, u32 level, u32 batch, u32 pass_override) {
  if (batch == 0) return 0;
  const u64 per = (u64)2 * level * c->n * sizeof(u64);
  u64 p = std::max<u64>(1, kEncPassBytes / per);
  if (pass_override) p = std::min<u64>(p, pass_override);
  return (u32)std::min<u64>(batch, p);
}

size_t encrypt_workspace_bytes(const fhe_ctx* c, u32 level, u32 batch) {
  return enc_ws(c, nullptr, level, encrypt_pass_batch(c, level, batch, 0)).words * sizeof(u64);
}

int launch_encrypt(const fhe_ctx* c, const EncryptArgs& a, void* ws, bool unfused, u32 pass_override,
                   hipStream_t s) {
  const u64 n = c->n;
  const u32 level = a.level, row_pairs = (u32)(n / 2);  // N >= 2^10: whole pairs per row
  const u32 pass = encrypt_pass_batch(c, level, a.batch, pass_override);
  const u32 gx = (row_pairs + kEncThreads - 1) / kEncThreads;
  const bool spread = c->wide || unfused;
  const u64 ln = (u64)level * n;
  int rc;
  for (u32 i0 = 0; i0 < a.batch; i0 += pass) {
    const u32 b = std::min(pass, a.batch - i0);
    const EncWs w = enc_ws(c, static_cast<u64*>(ws), level, b);
    u64* ct = a.ct + (u64)i0 * 2 * ln;
    const long long* msg = nullptr;
    if (a.slots) {
      long long* cf = reinterpret_cast<long long*>(w.cf);
      if ((rc = launch_encode_coeffs(c, cf, a.slots + ((u64)i0 << (a.log_slots + 1)), a.delta,
                                     a.log_slots, b, w.draws, s)))
        return rc;
      msg = cf;
    }
    EncDraw d{};
    d.u = reinterpret_cast<long long*>(w.draws);
    d.e = reinterpret_cast<long long*>(a.secret ? w.draws : w.draws + (u64)b * n);
    d.msg = msg;
    d.nd = a.secret ? 1 : 3;
    d.batch = b;
    d.row_pairs = row_pairs;
    d.poly0 = a.index0 + i0;
    d.seed_lo = (u32)a.seed;
    d.seed_hi = (u32)(a.seed >> 32);
    const u64 drows = (u64)d.nd * b;
    k_enc_draw<<<dim3(gx, (u32)std::min<u64>(drows, kMaxGridYZ)), kEncThreads, 0, s>>>(d);
    FHE_HIP_CHECK(hipGetLastError());
    prof_mark(s, "enc_draw");
    // e0, e1 -> the rows of c0, c1 and u -> that; the secret-key form's e -> that
    const long long* ecf = d.e;
    const long long* tcf = a.secret ? d.e : d.u;
    if (spread) {
      if (!a.secret &&
          ((rc = launch_encode_spread(c, ct, ecf, level, level, 2 * b, s)) ||
           (rc = launch_ntt(c, true, ct, ct, 2 * b, ln, 0, level, s))))
        return rc;
      if ((rc = launch_encode_spread(c, w.that, tcf, level, level, b, s)) ||
          (rc = launch_ntt(c, true, w.that, w.that, b, ln, 0, level, s)))
        return rc;
    } else {
      if (!a.secret &&
          ((rc = launch_encode_col(c, reinterpret_cast<const u64*>(ecf), ct, 2 * b, level, level,
                                   s)) ||
           (rc = launch_ntt_row_fwd_r2(c, ct, ln, ct, ln, 2 * b, 0, level, s))))
        return rc;
      if ((rc = launch_encode_col(c, reinterpret_cast<const u64*>(tcf), w.that, b, level, level,
                                  s)) ||
          (rc = launch_ntt_row_fwd_r2(c, w.that, ln, w.that, ln, b, 0, level, s)))
        return rc;
    }
    prof_mark(s, "enc_ntt");
    EncFinish f{};
    f.ct = ct;
    f.that = w.that;
    f.key0 = a.key;
    f.key1 = a.key + (u64)c->L * n;
    f.pt = a.pt ? a.pt + (a.pt_batch == 1 ? 0 : (u64)i0 * a.pt_rows * n) : nullptr;
    f.pt_bs = a.pt_batch == 1 ? 0 : (u64)a.pt_rows * n;
    f.level = level;
    f.nrows = b * level;  // pass <= kEncPassBytes / (2 level N words): far below 2^32
    f.row_pairs = row_pairs;
    f.poly0 = d.poly0;
    f.seed_lo = d.seed_lo;
    f.seed_hi = d.seed_hi;
    const dim3 g(gx, std::min<u32>(f.nrows, (u32)kMaxGridYZ));
    if (a.secret)
      k_enc_finish<true><<<g, kEncThreads, 0, s>>>(f, c->d_mods);
    else
      k_enc_finish<false><<<g, kEncThreads, 0, s>>>(f, c->d_mods);
    FHE_HIP_CHECK(hipGetLastError());
    prof_mark(s, "enc_finish");
  }
  return kOk;
}

}  // namespace fhe

using namespace fhe;

extern "C" {

int fhe_sample(const fhe_ctx* c, uint64_t* out, uint32_t polys, uint32_t limb0, uint32_t nlimbs,
               int kind, uint64_t seed, uint32_t tag, fhe_stream_t s) {
  if (!c || (uint64_t)limb0 + nlimbs > c->moduli.size() || kind < 0 || kind > 2) {
    set_error("fhe_sample: null context, limb window out of range or unknown kind");
    return kInvalid;
  }
  return sample(c, out, (u64)nlimbs * c->n, polys, limb0, nlimbs, kind, seed, tag,
                static_cast<hipStream_t>(s));
}

int fhe_keygen_secret(const fhe_ctx* c, uint64_t* sk, uint64_t seed, fhe_stream_t st) {
  if (!c) return (set_error("fhe_keygen_secret: null context"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 M = (u32)c->moduli.size();
  int rc;
  if ((rc = sample(c, sk, (u64)M * c->n, 1, 0, M, kTernary, seed, kTagSecret, s))) return rc;
  return launch_ntt(c, true, sk, sk, 1, (u64)M * c->n, 0, M, s);
}

int fhe_keygen_secret_sparse(const fhe_ctx* c, uint64_t* sk, uint32_t h, uint64_t seed,
                             fhe_stream_t st) {
  if (!c || !sk) return (set_error("fhe_keygen_secret_sparse: null context or output"), kInvalid);
  if (h == 0 || h > c->n)
    return (set_error("fhe_keygen_secret_sparse: the Hamming weight must be in [1, N]"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 M = (u32)c->moduli.size();
  if (int rc = check_grid(c->n / kThreads, kThreads, M, 1, "keygen_secret_sparse")) return rc;
  k_sparse_select<<<1, kSelThreads, 0, s>>>(sk + (u64)(M - 1) * c->n, (u32)c->n, h, (u32)seed,
                                            (u32)(seed >> 32), c->moduli[M - 1]);
  FHE_HIP_CHECK(hipGetLastError());
  if (M > 1) {
    k_sparse_spread<<<dim3((u32)(c->n / kThreads), M - 1), kThreads, 0, s>>>(sk, c->log_n, M - 1,
                                                                            c->d_mods);
    FHE_HIP_CHECK(hipGetLastError());
  }
  return launch_ntt(c, true, sk, sk, 1, (u64)M * c->n, 0, M, s);
}

int fhe_keygen_public(const fhe_ctx* c, uint64_t* pk, const uint64_t* sk, uint64_t seed,
                      fhe_stream_t st) {
  if (!c) return (set_error("fhe_keygen_public: null context"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 L = c->L;
  const u64 ln = (u64)L * c->n;
  u64* b = pk;       // b = -a s + e
  u64* a = pk + ln;  // uniform, NTT form
  int rc;
  if ((rc = sample(c, a, ln, 1, 0, L, kUniform, seed, kTagPkA, s)) ||
      (rc = sample(c, b, ln, 1, 0, L, kError, seed, kTagPkE, s)) ||
      (rc = launch_ntt(c, true, b, b, 1, ln, 0, L, s)))
    return rc;
  return mac_s(c, b, ln, b, ln, a, ln, sk, 1, 0, L, true, s);
}

// evk_j = (-a_j s + e_j + P g_j s_from, a_j) over Q u P, NTT form; key [2][dnum][L + K][N]
// (b part then a part).  g_j = 1 mod the primes of digit j, 0 mod the other Q-primes; P g_j
// is 0 mod every P-prime, so the P rows carry only -a_j s + e_j.
int fhe_keygen_switch(const fhe_ctx* c, uint64_t* key, const uint64_t* sk, const uint64_t* s_from,
                      uint64_t seed, fhe_stream_t st) {
  if (!c || c->K == 0) return (set_error("fhe_keygen_switch: needs a context with K > 0"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 L = c->L, M = L + c->K, dnum = c->dnum, alpha = c->alpha;
  const u64 mn = (u64)M * c->n;
  u64* kb = key;
  u64* ka = key + (u64)dnum * mn;
  int rc;
  for (u32 j = 0; j < dnum; ++j) {
    u64* b = kb + j * mn;
    u64* a = ka + j * mn;
    if ((rc = sample(c, a, mn, 1, 0, M, kUniform, seed, kTagKsA + 2 * j, s)) ||
        (rc = sample(c, b, mn, 1, 0, M, kError, seed, kTagKsE + 2 * j, s)) ||
        (rc = launch_ntt(c, true, b, b, 1, mn, 0, M, s)) ||
        (rc = mac_s(c, b, mn, b, mn, a, mn, sk, 1, 0, M, true, s)))
      return rc;
    // + P g_j s_from on the Q-limbs of digit j: P g_j = P mod q_i there, 0 on the other Q-limbs
    const u32 lo = j * alpha, hi = std::min(L, lo + alpha);
    for (u32 i = lo; i < hi; ++i) {
      const u64 q = c->moduli[i];
      u64 pm = 1;
      for (u32 k = 0; k < c->K; ++k) pm = mulmod_u64(pm, c->moduli[L + k] % q, q);
      k_axpy_const<<<(u32)(c->n / kThreads), kThreads, 0, s>>>(
          b + (u64)i * c->n, s_from + (u64)i * c->n, pm, (u64)(((u128)pm << 64) / q), q);
      FHE_HIP_CHECK(hipGetLastError());
    }
  }
  return kOk;
}

// Public-key encryption of an NTT-form plaintext pt [L][N]: c0 = b u + e0 + pt, c1 = a u + e1.
int fhe_encrypt(const fhe_ctx* c, uint64_t* ct, const uint64_t* pt, const uint64_t* pk,
                uint64_t seed, void* ws, fhe_stream_t st) {
  if (!c) return (set_error("fhe_encrypt: null context"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 L = c->L;
  const u64 ln = (u64)L * c->n;
  int rc0 = ensure_ws(c, ln * sizeof(u64), &ws, s);
  if (rc0) return rc0;
  u64* u = static_cast<u64*>(ws);  // [L][N]
  u64* c0 = ct;
  u64* c1 = ct + ln;
  int rc;
  if ((rc = sample(c, u, ln, 1, 0, L, kTernary, seed, kTagEncU, s)) ||
      (rc = launch_ntt(c, true, u, u, 1, ln, 0, L, s)) ||
      (rc = sample(c, c0, ln, 1, 0, L, kError, seed, kTagEncE0, s)) ||
      (rc = sample(c, c1, ln, 1, 0, L, kError, seed, kTagEncE1, s)) ||
      (rc = launch_ntt(c, true, c0, c0, 2, ln, 0, L, s)) ||
      (rc = mac_s(c, c0, ln, c0, ln, pk, ln, u, 1, 0, L, false, s)) ||        // + b u
      (rc = mac_s(c, c1, ln, c1, ln, pk + ln, ln, u, 1, 0, L, false, s)) ||   // + a u
      (rc = launch_vec_ctx(c, kAdd, c0, c0, pt, 1, 0, L, s)))
    return rc;
  return kOk;
}

// Secret-key encryption: c1 = a (uniform), c0 = -a s + e + pt.
int fhe_encrypt_sk(const fhe_ctx* c, uint64_t* ct, const uint64_t* pt, const uint64_t* sk,
                   uint64_t seed, fhe_stream_t st) {
  if (!c) return (set_error("fhe_encrypt_sk: null context"), kInvalid);
  const hipStream_t s = static_cast<hipStream_t>(st);
  const u32 L = c->L;
  const u64 ln = (u64)L * c->n;
  int rc;
  if ((rc = sample(c, ct + ln, ln, 1, 0, L, kUniform, seed, kTagEncA, s)) ||
      (rc = sample(c, ct, ln, 1, 0, L, kError, seed, kTagEncE, s)) ||
      (rc = launch_ntt(c, true, ct, ct, 1, ln, 0, L, s)) ||
      (rc = mac_s(c, ct, ln, ct, ln, ct + ln, ln, sk, 1, 0, L, true, s)) ||
      (rc = launch_vec_ctx(c, kAdd, ct, ct, pt, 1, 0, L, s)))
    return rc;
  return kOk;
}

// pt = c0 + c1 s over the first nlimbs Q-limbs (a ciphertext at any level), NTT form; batch
// ciphertexts [batch][2][nlimbs][N] -> [batch][nlimbs][N].
int fhe_decrypt(const fhe_ctx* c, uint64_t* pt, const uint64_t* ct, const uint64_t* sk,
                uint32_t batch, uint32_t nlimbs, fhe_stream_t st) {
  if (!c || nlimbs == 0 || nlimbs > c->L)
    return (set_error("fhe_decrypt: null context or nlimbs outside [1, L]"), kInvalid);
  const u64 ln = (u64)nlimbs * c->n;
  return mac_s(c, pt, ln, ct, 2 * ln, ct + ln, 2 * ln, sk, batch, 0, nlimbs, false,
               static_cast<hipStream_t>(st));
}

}  // extern "C"
