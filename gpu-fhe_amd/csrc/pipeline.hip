// Fused multiply -> relinearise -> rescale pipeline and HIP-graph capture:
// the CKKS ct x ct product as it is used in practice, everything in NTT form:
//   d = (a0 b0, a0 b1 + a1 b0, a1 b1)            elementwise tensor (k_tensor_ntt)
//   (ks0, ks1) = KeySwitch(d2, relin key)          the batched hybrid key-switch (rns.hip)
//   ct = (d0 + ks0, d1 + ks1)                      folded into the key-switch's ModDown finish
//                                                  (KsEpilogue: no separate combine pass)
//   [optional] ct = Rescale(ct)                    divide-and-round by the last modulus (galois.hip)
// fhe_mul_sum_relin_level is the same pipeline with the sum of up to 16 tensors in d's place
// (k_tensor_sum_ntt): one key-switch and one rescale for a whole sum of products.
// Restated by oracle/pyoracle.py (mul_relin); not in the reference, whose only ciphertext
// operation is poly_add (/root/reference/ polynomial.py:3-5).  The launches never allocate or
// synchronise given a workspace, so the whole pipeline can be captured into a hipGraph once and
// replayed (fhe_graph_*), removing per-launch host overhead from repeated small-batch calls.
#include "../../include/fhecore.h"
#include "internal.hpp"

namespace fhe {
namespace {


// a, b [batch][2][L][N] NTT form, canonical -> d0, d1 into d [batch][2][L][N] and d2 into its own
// contiguous [batch][L][N] (the key-switch's operand, no gather copy).  Grid: x over coefficient
// pairs (16-byte accesses), y = limb, z = ciphertext.  a, b are read once and d0, d1 are read back
// only by the key-switch's finish, long after they left the caches: non-temporal; d2 stays cached
// for the INTT that reads it next.
typedef u64 vu64x2 __attribute__((ext_vector_type(2)));
constexpr int kTensorThreads = 128;
__global__ __launch_bounds__(kTensorThreads) void k_tensor_ntt(u64* __restrict__ d,
                                                               u64* __restrict__ d2,
                                                               const u64* __restrict__ a,
                                                               const u64* __restrict__ b, u32 L,
                                                               u32 log_n,
                                                               const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n, ln = (u64)L * n;
  const u64 c = 2 * ((u64)blockIdx.x * blockDim.x + threadIdx.x);
  const u32 l = blockIdx.y;
  const u64 bt = blockIdx.z;
  const ModParams m = mods[l];
  const u64 off = bt * 2 * ln + (u64)l * n + c;
  auto ld = [](const u64* p) { return __builtin_nontemporal_load(reinterpret_cast<const vu64x2*>(p)); };
  const vu64x2 a0 = ld(a + off), a1 = ld(a + off + ln), b0 = ld(b + off), b1 = ld(b + off + ln);
  vu64x2 o0, o1, o2;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u128 t0 = (u128)a0[h] * b0[h], t2 = (u128)a1[h] * b1[h];
    const u128 t1 = (u128)a0[h] * b1[h] + (u128)a1[h] * b0[h];
    o0[h] = reduce128_any((u64)t0, (u64)(t0 >> 64), m);
    o1[h] = reduce128_any((u64)t1, (u64)(t1 >> 64), m);
    o2[h] = reduce128_any((u64)t2, (u64)(t2 >> 64), m);
  }
  u64* o = d + bt * 2 * ln + (u64)l * n + c;
  __builtin_nontemporal_store(o0, reinterpret_cast<vu64x2*>(o));
  __builtin_nontemporal_store(o1, reinterpret_cast<vu64x2*>(o + ln));
  *reinterpret_cast<vu64x2*>(d2 + bt * ln + (u64)l * n + c) = o2;
}

// The sum of `count` tensors in one pass (fhe_mul_sum_relin_level): D_k = sum_i d_k(a_i, b_i) for
// k = 0, 1, 2, D_0 and D_1 into d and D_2 into d2 exactly as k_tensor_ntt leaves its one tensor.
// Same grid (x over coefficient pairs, y = limb: ModParams wave-uniform, z = ciphertext).  Term i
// is read through its own strides (a_i at level la_i: polynomials la_i N apart, ciphertexts
// 2 la_i N), so a term above `level` is cut to it at no cost; the pointers and strides travel in
// the kernel arguments (uniform: scalar loads), nothing is staged on the device.  Every operand
// word is read once, non-temporally, kTensorGroup terms' loads issued before the group's first
// product; 8 (4 count + 3) bytes per element.  The inputs may alias each other in any way (they
// are only read); d and d2 are workspace.
// Accumulation:
//  * narrow (every context modulus < 2^61): products < 2^122 summed in 128 bits -- D_1 takes two
//    per term, 32 q^2 < 2^127 at 16 terms -- and one reduce128 per component whatever the count;
//  * wide (some modulus in [2^61, 2^63)): each term (a0 b1 + a1 b0 < 2 q^2 < 2^127) reduced to
//    [0, q) by reduce128_any, then added with one conditional subtraction (< 2q < 2^64).
// Both return the canonical residue, so the result does not depend on the order of the terms.
constexpr u32 kTensorGroup = 4;
struct TensorSumArgs {
  const u64* a[kMulSumMax];
  const u64* b[kMulSumMax];
  u64 as[kMulSumMax], bs[kMulSumMax];  // words between the two polynomials of a_i / b_i
  u32 count;
};
template <bool WIDE>
__global__ __launch_bounds__(kTensorThreads) void k_tensor_sum_ntt(u64* __restrict__ d,
                                                                   u64* __restrict__ d2,
                                                                   const TensorSumArgs t, u32 L,
                                                                   u32 log_n,
                                                                   const ModParams* __restrict__ mods) {
  const u64 n = 1ull << log_n, ln = (u64)L * n;
  const u64 c = 2 * ((u64)blockIdx.x * blockDim.x + threadIdx.x);
  const u32 l = blockIdx.y;
  const u64 bt = blockIdx.z;
  const ModParams m = mods[l];
  const u64 off = (u64)l * n + c;
  auto ld = [](const u64* p) { return __builtin_nontemporal_load(reinterpret_cast<const vu64x2*>(p)); };
  u128 s[3][2] = {};  // narrow
  u64 w[3][2] = {};   // wide
  for (u32 i0 = 0; i0 < t.count; i0 += kTensorGroup) {
    vu64x2 a0[kTensorGroup], a1[kTensorGroup], b0[kTensorGroup], b1[kTensorGroup];
#pragma unroll
    for (u32 u = 0; u < kTensorGroup; ++u) {
      const u32 i = i0 + u;
      if (i < t.count) {
        const u64* pa = t.a[i] + bt * 2 * t.as[i] + off;
        const u64* pb = t.b[i] + bt * 2 * t.bs[i] + off;
        a0[u] = ld(pa), a1[u] = ld(pa + t.as[i]), b0[u] = ld(pb), b1[u] = ld(pb + t.bs[i]);
      }
    }
#pragma unroll
    for (u32 u = 0; u < kTensorGroup; ++u) {
      if (i0 + u < t.count) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const u128 t0 = (u128)a0[u][h] * b0[u][h], t2 = (u128)a1[u][h] * b1[u][h];
          const u128 t1 = (u128)a0[u][h] * b1[u][h] + (u128)a1[u][h] * b0[u][h];
          if constexpr (WIDE) {
            w[0][h] = csub(w[0][h] + reduce128_any((u64)t0, (u64)(t0 >> 64), m), m.q);
            w[1][h] = csub(w[1][h] + reduce128_any((u64)t1, (u64)(t1 >> 64), m), m.q);
            w[2][h] = csub(w[2][h] + reduce128_any((u64)t2, (u64)(t2 >> 64), m), m.q);
          } else {
            s[0][h] += t0, s[1][h] += t1, s[2][h] += t2;
          }
        }
      }
    }
  }
  vu64x2 o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      o[k][h] = WIDE ? w[k][h] : reduce128((u64)s[k][h], (u64)(s[k][h] >> 64), m);
  u64* po = d + bt * 2 * ln + off;
  __builtin_nontemporal_store(o[0], reinterpret_cast<vu64x2*>(po));
  __builtin_nontemporal_store(o[1], reinterpret_cast<vu64x2*>(po + ln));
  *reinterpret_cast<vu64x2*>(d2 + bt * ln + off) = o[2];
}

// The workspace of launch_mul_relin at `level` live Q-limbs (ws null: the size only)
struct MulRelinWs {
  u64 *d, *rl;  // [batch][2][level][N] each: d0, d1; the relinearised ct before the rescale
  // [batch][level][N] d2, NTT form, the key-switch's input (its finish may run in the same kernel
  // as its reads of d2, k_ks_row_fin, so d2 cannot park in the output)
  u64* d2;
  u64* rws;  // the rescale's own workspace
  u64* kws;  // the key-switch's workspace (ks: its plan; the tail holds INTT(d2))
  KsPlan ks;
  size_t bytes;
};
MulRelinWs mul_relin_ws(const fhe_ctx* c, void* ws, u32 level, u32 batch) {
  const u64 ln = (u64)level * c->n;
  WsCarve w{static_cast<u64*>(ws)};
  MulRelinWs r;
  r.d = w.take(2 * batch * ln);
  r.rl = w.take(2 * batch * ln);
  r.d2 = w.take(batch * ln);
  r.rws = w.take(rescale_workspace_bytes(c, 2 * batch, level) / sizeof(u64));
  r.ks = ks_plan_level(c, level, batch);
  r.kws = w.take(r.ks.total);
  r.bytes = w.bytes();
  return r;
}

// The tail shared by launch_mul_relin and launch_mul_sum_relin once the tensor (d0, d1 in w.d, d2
// in w.d2) is in the workspace: INTT(d2), the key-switch with (d0, d1) as its finish's addends,
// the optional rescale.
int relin_tail(const fhe_ctx* c, const MulRelinWs& w, u64* out, const u64* evk_b, const u64* evk_a,
               u32 L, u32 batch, bool rescale, hipStream_t s) {
  const u64 ln = (u64)L * c->n;
  u64 *d = w.d, *d2 = w.d2;
  // d2 = d[b][2]: gather to a contiguous [batch][L][N] operand for the key-switch (its INTT lands
  // at the tail of the key-switch workspace, as in fhe_keyswitch)
  int rc;
  CAll call{};
  if ((rc = ks_input_intt(c, w.ks, d2, ln, w.kws + w.ks.call, ln, batch, s, &call))) return rc;
  // the relinearised ciphertext (d0 + ks0, d1 + ks1) straight out of the ModDown finish
  // ([batch][2][L][N] outputs and addends, 2 L N apart per ciphertext)
  u64* dst = rescale ? w.rl : out;
  KsEpilogue ep;
  ep.out_bs = 2 * ln;
  ep.add0 = d;
  ep.add1 = d + ln;
  ep.add_bs = 2 * ln;
  if ((rc = launch_keyswitch_shard(c, dst, dst + ln, call, d2, evk_b, evk_a, 0, L, batch, w.kws,
                                   s, &ep, nullptr, L)))
    return rc;
  prof_mark(s, "relin_keyswitch");
  if (rescale) {
    if ((rc = launch_rescale(c, out, w.rl, 2 * batch, L, true, w.rws, s))) return rc;
    prof_mark(s, "rescale");
  }
  return kOk;
}

// what both launchers require of the context, the level and the rescale flag
int check_mul_relin(const fhe_ctx* c, u32 level, bool rescale, const char* who) {
  if (c->K == 0) {
    set_error(std::string(who) + ": context has no special primes (K = 0)");
    return kInvalid;
  }
  if (level == 0 || level > c->L) {
    set_error(std::string(who) + ": level must be in [1, L]");
    return kInvalid;
  }
  if (rescale && level < 2) {
    set_error(std::string(who) + ": rescale needs at least 2 limbs");
    return kInvalid;
  }
  return kOk;
}

}  // namespace

size_t mul_relin_workspace_bytes(const fhe_ctx* c, u32 batch) {
  return mul_relin_ws(c, nullptr, c->L, batch).bytes;
}

// `level` Q-limbs (1 .. c->L) in a, b and out: the workspace regions are laid out for that many,
// so mul_relin_workspace_bytes (sized for c->L) covers every level.
int launch_mul_relin(const fhe_ctx* c, u64* out, const u64* a, const u64* b, const u64* evk_b,
                     const u64* evk_a, u32 level, u32 batch, bool rescale, void* ws,
                     hipStream_t s) {
  if (int rc = check_mul_relin(c, level, rescale, "mul_relin")) return rc;
  if (batch == 0) return kOk;
  const u32 L = level;  // the live Q-limbs
  const u64 n = c->n, ln = (u64)L * n;
  // Infinity-Cache-sized passes (ks_pass_batch), each in the front of the workspace
  if (const u32 pass = ks_pass_batch(c, batch); pass < batch) {
    const u64 out_bs = 2 * (u64)(rescale ? L - 1 : L) * n;
    for (u32 b0 = 0; b0 < batch; b0 += pass) {
      if (int rc = launch_mul_relin(c, out + b0 * out_bs, a + b0 * 2 * ln, b + b0 * 2 * ln, evk_b,
                                    evk_a, level, std::min(pass, batch - b0), rescale, ws, s))
        return rc;
    }
    return kOk;
  }
  const MulRelinWs w = mul_relin_ws(c, ws, level, batch);
  const u64 tb = n / 2 / kTensorThreads;  // N >= 2^10: whole blocks of coefficient pairs
  if (int rc = check_grid(tb, kTensorThreads, L, batch, "tensor_ntt")) return rc;
  const dim3 g((u32)tb, L, batch);
  k_tensor_ntt<<<g, kTensorThreads, 0, s>>>(w.d, w.d2, a, b, L, c->log_n, c->d_mods);
  FHE_HIP_CHECK(hipGetLastError());
  prof_mark(s, "tensor_ntt");
  return relin_tail(c, w, out, evk_b, evk_a, L, batch, rescale, s);
}

// The sum of count products relinearised once: launch_mul_relin with k_tensor_sum_ntt in the
// tensor's place (same workspace regions, same passes; each term advances by its own stride).
int launch_mul_sum_relin(const fhe_ctx* c, u64* out, const u64* const* a, const u32* a_levels,
                         const u64* const* b, const u32* b_levels, const u64* evk_b,
                         const u64* evk_a, u32 level, u32 count, u32 batch, bool rescale,
                         void* ws, hipStream_t s) {
  if (int rc = check_mul_relin(c, level, rescale, "mul_sum_relin")) return rc;
  if (count == 0 || count > kMulSumMax) {
    set_error("mul_sum_relin: count must be 1..16");
    return kInvalid;
  }
  if (batch == 0) return kOk;
  // one product of operands already at `level` is launch_mul_relin itself: k_tensor_ntt, whose
  // pass is ~1.5 % shorter than the general kernel's with one term (0.287 against 0.291 ms at
  // N = 2^16, level 16, batch 32), so the one-term call costs what fhe_mul_relin_level costs
  if (count == 1 && a_levels[0] == level && b_levels[0] == level)
    return launch_mul_relin(c, out, a[0], b[0], evk_b, evk_a, level, batch, rescale, ws, s);
  const u32 L = level;
  const u64 n = c->n;
  const u64 out_bs = 2 * (u64)(rescale ? L - 1 : L) * n;
  const u64 tb = n / 2 / kTensorThreads;  // N >= 2^10: whole blocks of coefficient pairs
  const u32 pass = ks_pass_batch(c, batch);
  for (u32 b0 = 0; b0 < batch; b0 += pass) {
    const u32 bn = std::min(pass, batch - b0);
    TensorSumArgs t{};
    t.count = count;
    for (u32 i = 0; i < count; ++i) {
      t.as[i] = (u64)a_levels[i] * n;
      t.bs[i] = (u64)b_levels[i] * n;
      t.a[i] = a[i] + b0 * 2 * t.as[i];
      t.b[i] = b[i] + b0 * 2 * t.bs[i];
    }
    const MulRelinWs w = mul_relin_ws(c, ws, level, bn);
    if (int rc = check_grid(tb, kTensorThreads, L, bn, "tensor_sum_ntt")) return rc;
    const dim3 g((u32)tb, L, bn);
    if (c->wide)
      k_tensor_sum_ntt<true><<<g, kTensorThreads, 0, s>>>(w.d, w.d2, t, L, c->log_n, c->d_mods);
    else
      k_tensor_sum_ntt<false><<<g, kTensorThreads, 0, s>>>(w.d, w.d2, t, L, c->log_n, c->d_mods);
    FHE_HIP_CHECK(hipGetLastError());
    prof_mark(s, "tensor_sum_ntt");
    if (int rc = relin_tail(c, w, out + b0 * out_bs, evk_b, evk_a, L, bn, rescale, s)) return rc;
  }
  return kOk;
}

}  // namespace fhe

// ---- HIP graphs: capture any sequence of libfhecore calls on a stream, replay it -------------
extern "C" {

int fhe_graph_begin(fhe_stream_t stream) {
  FHE_HIP_CHECK(hipStreamBeginCapture(static_cast<hipStream_t>(stream),
                                      hipStreamCaptureModeThreadLocal));
  return fhe::kOk;
}

int fhe_graph_end(fhe_stream_t stream, fhe_graph_t* graph) {
  if (!graph) {
    fhe::set_error("fhe_graph_end: null graph pointer");
    return fhe::kInvalid;
  }
  *graph = nullptr;
  hipGraph_t g = nullptr;
  FHE_HIP_CHECK(hipStreamEndCapture(static_cast<hipStream_t>(stream), &g));
  hipGraphExec_t ge = nullptr;
  const hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    fhe::set_error(std::string("fhe_graph_end: hipGraphInstantiate: ") + hipGetErrorString(e));
    return fhe::kDevice;
  }
  *graph = reinterpret_cast<fhe_graph_t>(ge);
  return fhe::kOk;
}

int fhe_graph_launch(fhe_graph_t graph, fhe_stream_t stream) {
  if (!graph) {
    fhe::set_error("fhe_graph_launch: null graph");
    return fhe::kInvalid;
  }
  FHE_HIP_CHECK(hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph),
                               static_cast<hipStream_t>(stream)));
  return fhe::kOk;
}

int fhe_graph_destroy(fhe_graph_t graph) {
  if (graph) FHE_HIP_CHECK(hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(graph)));
  return fhe::kOk;
}

}  // extern "C"
