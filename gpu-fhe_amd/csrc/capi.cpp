// extern "C" entry points of libfhecore (declared in include/fhecore.h): argument checking,
// error reporting and workspace handling around the HIP launchers.
#include "../../include/fhecore.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>

#include "internal.hpp"

namespace fhe {

namespace {
thread_local std::string g_last_error;

inline hipStream_t hs(fhe_stream_t s) { return static_cast<hipStream_t>(s); }

int check_window(const fhe_ctx* c, uint32_t limb0, uint32_t nlimbs, uint32_t limit,
                 const char* who) {
  if (!c) {
    set_error(std::string(who) + ": null context");
    return kInvalid;
  }
  if ((uint64_t)limb0 + nlimbs > limit) {
    set_error(std::string(who) + ": limb window [" + std::to_string(limb0) + ", " +
              std::to_string(limb0 + nlimbs) + ") exceeds " + std::to_string(limit) + " limbs");
    return kInvalid;
  }
  return kOk;
}

}  // namespace

// Internal workspace (grows on demand).  Refused while `s` is capturing a graph: growing it would
// free memory a captured graph still points at, and a graph sharing it with eager calls on other
// streams would race them, so captured calls must bring their own workspace.
// Calls on different streams are ordered: a call whose stream differs from the last user's first
// waits (host side, hipDeviceSynchronize) until the device has finished what was queued before it,
// which includes the last call's launches since calls sharing the internal workspace are issued
// one after another by the host (concurrent host threads must pass their own workspaces,
// fhecore.h).  The last user's stream is not touched again: the caller may have destroyed it.
// Growing the buffer waits the same way before the old one is freed.  The waits, frees and
// allocations run on the context's device whatever device the calling thread has current
// (DeviceScope), so a multi-GPU host thread cannot wait on, or allocate from, the wrong GPU.
// use = false (fhe_ctx_reserve) only sizes the buffer: no stream takes it.
namespace {

// Makes `dev` current for the scope and restores the caller's device after.
struct DeviceScope {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && prev != dev) err = hipSetDevice(dev);
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

int acquire_ws(fhe_ctx* c, size_t bytes, hipStream_t s, bool use) {
  DeviceScope dev(c->device);
  FHE_HIP_CHECK(dev.err);
  std::lock_guard<std::mutex> lock(c->ws_mutex);
  const bool grow = c->workspace_bytes < bytes;
  if (c->ws_used && ((use && c->ws_stream != s) || grow)) FHE_HIP_CHECK(hipDeviceSynchronize());
  if (grow) {
    if (c->workspace) FHE_HIP_CHECK(hipFree(c->workspace));
    c->workspace = nullptr;
    c->workspace_bytes = 0;
    FHE_HIP_CHECK(hipMalloc(&c->workspace, bytes));
    c->workspace_bytes = bytes;
  }
  if (use) {
    c->ws_stream = s;
    c->ws_used = true;
  }
  return kOk;
}

}  // namespace

int ensure_ws(const fhe_ctx* cc, size_t bytes, void** ws, hipStream_t s) {
  if (*ws) return kOk;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  FHE_HIP_CHECK(hipStreamIsCapturing(s, &st));
  if (st != hipStreamCaptureStatusNone) {
    set_error("workspace == NULL while the stream is capturing a graph: pass a workspace");
    return kInvalid;
  }
  auto* c = const_cast<fhe_ctx*>(cc);
  int rc = acquire_ws(c, bytes, s, true);
  if (rc) return rc;
  *ws = c->workspace;
  return kOk;
}

void set_error(const std::string& msg) { g_last_error = msg; }

}  // namespace fhe

using namespace fhe;

extern "C" {

const char* fhe_last_error(void) { return g_last_error.c_str(); }

const char* fhe_version(void) { return "fhecore 0.1 (gfx950)"; }

int fhe_gen_moduli(uint32_t log_n, uint32_t count, uint32_t bits, uint32_t skip, uint64_t* out) {
  if (!out && count) {
    set_error("fhe_gen_moduli: null output");
    return kInvalid;
  }
  return gen_moduli(log_n, count, bits, skip, out);
}

int fhe_ctx_create(fhe_ctx** ctx, uint32_t log_n, const uint64_t* q, uint32_t L,
                   const uint64_t* p, uint32_t K, uint32_t dnum, int device) {
  if (!q || (K && !p)) {
    set_error("fhe_ctx_create: null modulus array");
    return kInvalid;
  }
  try {
    return ctx_create(ctx, log_n, q, L, p, K, dnum, device);
  } catch (const std::exception& e) {
    set_error(std::string("fhe_ctx_create: ") + e.what());
    return kNoMem;
  }
}

int fhe_ctx_destroy(fhe_ctx* ctx) { return ctx_destroy(ctx); }

int fhe_ctx_moduli(const fhe_ctx* c, uint64_t* moduli, uint64_t* psi) {
  if (!c) {
    set_error("fhe_ctx_moduli: null context");
    return kInvalid;
  }
  for (size_t i = 0; i < c->moduli.size(); ++i) {
    if (moduli) moduli[i] = c->moduli[i];
    if (psi) psi[i] = c->psi[i];
  }
  return kOk;
}

int fhe_ctx_shape(const fhe_ctx* c, uint32_t* log_n, uint32_t* L, uint32_t* K, uint32_t* dnum,
                  int* device) {
  if (!c) {
    set_error("fhe_ctx_shape: null context");
    return kInvalid;
  }
  if (log_n) *log_n = c->log_n;
  if (L) *L = c->L;
  if (K) *K = c->K;
  if (dnum) *dnum = c->dnum;
  if (device) *device = c->device;
  return kOk;
}

int fhe_ctx_reserve(fhe_ctx* c, size_t bytes) {
  if (!c) {
    set_error("fhe_ctx_reserve: null context");
    return kInvalid;
  }
  return acquire_ws(c, bytes, nullptr, false);
}

static int vec_ctx(int op, const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                   uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t s,
                   const char* who) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, who);
  if (rc) return rc;
  if ((!out || !a || !b) && (uint64_t)polys * nlimbs) {
    set_error(std::string(who) + ": null data pointer");
    return kInvalid;
  }
  return launch_vec_ctx(c, op, out, a, b, polys, limb0, nlimbs, hs(s));
}

int fhe_vec_add(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t s) {
  return vec_ctx(kAdd, c, out, a, b, polys, limb0, nlimbs, s, "fhe_vec_add");
}
int fhe_vec_sub(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t s) {
  return vec_ctx(kSub, c, out, a, b, polys, limb0, nlimbs, s, "fhe_vec_sub");
}
int fhe_vec_mul(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                uint32_t polys, uint32_t limb0, uint32_t nlimbs, fhe_stream_t s) {
  return vec_ctx(kMul, c, out, a, b, polys, limb0, nlimbs, s, "fhe_vec_mul");
}

int fhe_vec_op_mod(int op, uint64_t* out, const uint64_t* a, const uint64_t* b, uint64_t rows,
                   uint64_t cols, const uint64_t* mods, uint64_t mod_stride, int signed_in,
                   int device, fhe_stream_t s) {
  if (op < kAdd || op > kMul) {
    set_error("fhe_vec_op_mod: op must be 0 (add), 1 (sub) or 2 (mul)");
    return kInvalid;
  }
  if (rows * cols == 0) return kOk;
  if (!out || !a || !b || !mods) {
    set_error("fhe_vec_op_mod: null pointer");
    return kInvalid;
  }
  const uint64_t nm = mod_stride ? (rows - 1) * mod_stride + 1 : 1;
  for (uint64_t i = 0; i < nm; ++i)
    if (mods[i] < 2) {
      set_error("fhe_vec_op_mod: modulus must be >= 2");
      return kInvalid;
    }
  FHE_HIP_CHECK(hipSetDevice(device));
  if (nm <= (uint64_t)kArgMods) {  // the common case: moduli by value, nothing allocated or synced
    ModArgs inl{};
    for (uint64_t i = 0; i < nm; ++i) inl.m[i] = make_mod_params(mods[i]);
    return launch_vec_mod(op, out, a, b, rows, cols, nullptr, inl, mod_stride, signed_in, hs(s));
  }
  std::vector<ModParams> mp(nm);
  for (uint64_t i = 0; i < nm; ++i) mp[i] = make_mod_params(mods[i]);
  ModParams* d = nullptr;
  FHE_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&d), nm * sizeof(ModParams), hs(s)));
  FHE_HIP_CHECK(hipMemcpyAsync(d, mp.data(), nm * sizeof(ModParams), hipMemcpyHostToDevice, hs(s)));
  const int rc = launch_vec_mod(op, out, a, b, rows, cols, d, ModArgs{}, mod_stride, signed_in,
                                hs(s));
  FHE_HIP_CHECK(hipStreamSynchronize(hs(s)));  // mp must outlive the async copy
  FHE_HIP_CHECK(hipFreeAsync(d, hs(s)));
  return rc;
}

int fhe_ntt_fwd(const fhe_ctx* c, uint64_t* data, uint32_t polys, uint32_t limb0,
                uint32_t nlimbs, fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, "fhe_ntt_fwd");
  if (rc) return rc;
  return launch_ntt(c, true, data, data, polys, (uint64_t)nlimbs * c->n, limb0, nlimbs, hs(s));
}

int fhe_ntt_inv(const fhe_ctx* c, uint64_t* data, uint32_t polys, uint32_t limb0,
                uint32_t nlimbs, fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, "fhe_ntt_inv");
  if (rc) return rc;
  return launch_ntt(c, false, data, data, polys, (uint64_t)nlimbs * c->n, limb0, nlimbs, hs(s));
}

int fhe_ntt_fwd_to(const fhe_ctx* c, uint64_t* dst, const uint64_t* src, uint32_t polys,
                   uint32_t limb0, uint32_t nlimbs, fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, "fhe_ntt_fwd_to");
  if (rc) return rc;
  return launch_ntt(c, true, src, dst, polys, (uint64_t)nlimbs * c->n, limb0, nlimbs, hs(s));
}

int fhe_ntt_inv_to(const fhe_ctx* c, uint64_t* dst, const uint64_t* src, uint32_t polys,
                   uint32_t limb0, uint32_t nlimbs, fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, "fhe_ntt_inv_to");
  if (rc) return rc;
  return launch_ntt(c, false, src, dst, polys, (uint64_t)nlimbs * c->n, limb0, nlimbs, hs(s));
}

size_t fhe_hommult_workspace(const fhe_ctx* c, uint32_t batch, uint32_t nlimbs) {
  return c ? hommult_workspace_bytes(c, batch, nlimbs) : 0;
}

int fhe_hommult(const fhe_ctx* c, uint64_t* d, const uint64_t* a, const uint64_t* b,
                uint32_t batch, uint32_t limb0, uint32_t nlimbs, void* ws, fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L : 0, "fhe_hommult");
  if (rc) return rc;
  if ((rc = ensure_ws(c, hommult_workspace_bytes(c, batch, nlimbs), &ws, hs(s)))) return rc;
  return launch_hommult(c, d, a, b, batch, limb0, nlimbs, ws, hs(s));
}

int fhe_baseconv(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t s0, uint32_t S,
                 uint32_t t0, uint32_t T, fhe_stream_t s) {
  if (!c) {
    set_error("fhe_baseconv: null context");
    return kInvalid;
  }
  return launch_baseconv(c, out, in, s0, S, t0, T, hs(s));
}

size_t fhe_keyswitch_workspace(const fhe_ctx* c, uint32_t nlimbs, uint32_t batch) {
  return c ? keyswitch_workspace_bytes(c, nlimbs, batch) : 0;
}

uint32_t fhe_keyswitch_pass_batch(const fhe_ctx* c, uint32_t batch) {
  return c ? ks_pass_batch(c, batch) : 0;
}

int fhe_keyswitch_shard(const fhe_ctx* c, uint64_t* ks0, uint64_t* ks1, const uint64_t* c_all,
                        const uint64_t* d2_own, const uint64_t* evk_b, const uint64_t* evk_a,
                        uint32_t limb0, uint32_t nlimbs, uint32_t batch, void* ws,
                        fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L : 0, "fhe_keyswitch_shard");
  if (rc) return rc;
  if ((rc = ensure_ws(c, keyswitch_workspace_bytes(c, nlimbs, batch), &ws, hs(s)))) return rc;
  return launch_keyswitch_shard(c, ks0, ks1, CAll::contiguous(c_all, c->L, c->n), d2_own, evk_b,
                                evk_a, limb0, nlimbs, batch, ws, hs(s));
}

// The prologue of the *_level entry points: a context, and a level in [1, L] (so the limb window
// [0, level) lies inside the chain).
static int check_level(const fhe_ctx* c, uint32_t level, const char* who) {
  if (!c) {
    set_error(std::string(who) + ": null context");
    return kInvalid;
  }
  if (level == 0 || level > c->L) {
    set_error(std::string(who) + ": level must be in [1, L]");
    return kInvalid;
  }
  return kOk;
}

int fhe_keyswitch(const fhe_ctx* c, uint64_t* ks0, uint64_t* ks1, const uint64_t* d2,
                  const uint64_t* evk_b, const uint64_t* evk_a, uint32_t batch, void* ws,
                  fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_keyswitch");
  if (rc) return rc;
  return fhe_keyswitch_level(c, ks0, ks1, d2, evk_b, evk_a, c->L, batch, ws, s);
}

int fhe_keyswitch_level(const fhe_ctx* c, uint64_t* ks0, uint64_t* ks1, const uint64_t* d2,
                        const uint64_t* evk_b, const uint64_t* evk_a, uint32_t level,
                        uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_keyswitch_level");
  if (rc) return rc;
  if (batch == 0) return kOk;
  const uint64_t ct_words = (uint64_t)level * c->n;
  // the whole batch at once: a pass must not overwrite a later pass's d2 (per-pass checks in the
  // launcher would miss an output shifted onto the next pass's input)
  if ((rc = ks_check_alias(ks0, ks1, d2, batch * ct_words, batch * ct_words, true,
                           "fhe_keyswitch")))
    return rc;
  const uint32_t pass = ks_pass_batch(c, batch);  // Infinity-Cache-sized passes
  // the level's own regions: never more than fhe_keyswitch_workspace(ctx, L, pass)
  const KsPlan p = ks_plan_level(c, level, pass);
  if ((rc = ensure_ws(c, p.bytes(), &ws, hs(s)))) return rc;
  // c_all = INTT(d2) of one pass lives at the tail of the workspace (out of place: no copy of d2)
  uint64_t* c_all = static_cast<uint64_t*>(ws) + p.call;
  CAll src{};
  for (uint32_t b0 = 0; b0 < batch; b0 += pass) {
    const uint32_t bn = std::min(pass, batch - b0);
    const uint64_t off = (uint64_t)b0 * ct_words;
    if ((rc = ks_input_intt(c, p, d2 + off, ct_words, c_all, ct_words, bn, hs(s), &src))) return rc;
    if ((rc = launch_keyswitch_shard(c, ks0 + off, ks1 + off, src, d2 + off, evk_b, evk_a, 0, level,
                                     bn, ws, hs(s), nullptr, nullptr, level)))
      return rc;
  }
  return kOk;
}

size_t fhe_rescale_workspace(const fhe_ctx* c, uint32_t polys, uint32_t nlimbs) {
  return c ? rescale_workspace_bytes(c, polys, nlimbs) : 0;
}

int fhe_rescale(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t polys,
                uint32_t nlimbs, int ntt_form, void* ws, fhe_stream_t s) {
  int rc = check_window(c, 0, nlimbs, c ? c->L : 0, "fhe_rescale");
  if (rc) return rc;
  if (ntt_form && (rc = ensure_ws(c, rescale_workspace_bytes(c, polys, nlimbs), &ws, hs(s)))) return rc;
  return launch_rescale(c, out, in, polys, nlimbs, ntt_form != 0, ws, hs(s));
}

int fhe_automorphism(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t polys,
                     uint32_t limb0, uint32_t nlimbs, uint32_t galois_elt, int ntt_form,
                     fhe_stream_t s) {
  int rc = check_window(c, limb0, nlimbs, c ? c->L + c->K : 0, "fhe_automorphism");
  if (rc) return rc;
  if (out == in && polys && nlimbs) {
    set_error("fhe_automorphism: out must not alias in");
    return kInvalid;
  }
  const uint64_t stride = (uint64_t)nlimbs * c->n;
  return launch_automorphism(c, out, stride, in, stride, polys, limb0, nlimbs, galois_elt,
                             ntt_form != 0, hs(s));
}

size_t fhe_rotate_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? rotate_workspace_bytes(c, batch) : 0;
}

int fhe_rotate(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t galois_elt,
               const uint64_t* rot_b, const uint64_t* rot_a, uint32_t batch, void* ws,
               fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_rotate");
  if (rc) return rc;
  return fhe_rotate_level(c, out, in, galois_elt, rot_b, rot_a, c->L, batch, ws, s);
}

int fhe_rotate_level(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t galois_elt,
                     const uint64_t* rot_b, const uint64_t* rot_a, uint32_t level, uint32_t batch,
                     void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_rotate_level");
  if (rc) return rc;
  // the finish reads c0 through sigma (any word of its row block) while other workgroups write
  // out: any overlap of the two [batch][2][level][N] spans races, not just out == in
  const uint64_t span = (uint64_t)batch * 2 * level * c->n;
  if (spans_overlap(out, span, in, span)) {
    set_error("fhe_rotate: out must not overlap in");
    return kInvalid;
  }
  if ((rc = ensure_ws(c, rotate_workspace_bytes(c, ks_pass_batch(c, batch)), &ws, hs(s)))) return rc;
  return launch_rotate(c, out, in, galois_elt, rot_b, rot_a, level, batch, ws, hs(s));
}

size_t fhe_rotate_hoisted_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? rotate_hoisted_workspace_bytes(c, batch) : 0;
}

int fhe_rotate_hoisted(const fhe_ctx* c, uint64_t* out, const uint64_t* in,
                       const uint32_t* galois_elts, const uint64_t* const* rot_b,
                       const uint64_t* const* rot_a, uint32_t count, uint32_t batch, void* ws,
                       fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_rotate_hoisted");
  if (rc) return rc;
  return fhe_rotate_hoisted_level(c, out, in, galois_elts, rot_b, rot_a, c->L, count, batch, ws, s);
}

int fhe_rotate_hoisted_level(const fhe_ctx* c, uint64_t* out, const uint64_t* in,
                             const uint32_t* galois_elts, const uint64_t* const* rot_b,
                             const uint64_t* const* rot_a, uint32_t level, uint32_t count,
                             uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_rotate_hoisted_level");
  if (rc) return rc;
  if (count && (!galois_elts || !rot_b || !rot_a)) {
    set_error("fhe_rotate_hoisted: null Galois element or key array");
    return kInvalid;
  }
  for (uint32_t r = 0; r < count; ++r)
    if (!rot_b[r] || !rot_a[r]) {  // the kernels would dereference it on the device
      set_error("fhe_rotate_hoisted: null key pointer for rotation " + std::to_string(r));
      return kInvalid;
    }
  const uint64_t span = (uint64_t)count * batch * 2 * level * c->n;
  if (span && in < out + span && out < in + (uint64_t)batch * 2 * level * c->n) {
    set_error("fhe_rotate_hoisted: out must not overlap in");
    return kInvalid;
  }
  if ((rc = ensure_ws(c, rotate_hoisted_workspace_bytes(c, batch), &ws, hs(s)))) return rc;
  return launch_rotate_hoisted(c, out, in, galois_elts, rot_b, rot_a, level, count, batch, ws,
                               hs(s));
}

size_t fhe_rotate_sum_hoisted_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? rotate_sum_hoisted_workspace_bytes(c, batch) : 0;
}

int fhe_rotate_sum_hoisted(const fhe_ctx* c, uint64_t* out, const uint64_t* in,
                           const uint32_t* galois_elts, const uint64_t* const* rot_b,
                           const uint64_t* const* rot_a, const uint64_t* const* pt,
                           uint32_t count, uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_rotate_sum_hoisted");
  if (rc) return rc;
  return fhe_rotate_sum_hoisted_level(c, out, in, galois_elts, rot_b, rot_a, pt, c->L, count, batch,
                                      ws, s);
}

int fhe_rotate_sum_hoisted_level(const fhe_ctx* c, uint64_t* out, const uint64_t* in,
                                 const uint32_t* galois_elts, const uint64_t* const* rot_b,
                                 const uint64_t* const* rot_a, const uint64_t* const* pt,
                                 uint32_t level, uint32_t count, uint32_t batch, void* ws,
                                 fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_rotate_sum_hoisted_level");
  if (rc) return rc;
  if (count == 0 || count > kRotSumMax) {
    set_error("fhe_rotate_sum_hoisted: count must be 1..16");
    return kInvalid;
  }
  if (!galois_elts || !pt || ((!rot_b || !rot_a) && std::any_of(galois_elts, galois_elts + count,
                                                                 [](uint32_t g) { return g != 1; }))) {
    set_error("fhe_rotate_sum_hoisted: null Galois element, plaintext or key array");
    return kInvalid;
  }
  for (uint32_t r = 0; r < count; ++r) {
    // the kernels would dereference them on the device; the unrotated term (1) takes no key
    if (!pt[r] || (galois_elts[r] != 1 && (!rot_b[r] || !rot_a[r]))) {
      set_error("fhe_rotate_sum_hoisted: null plaintext or key pointer for term " +
                std::to_string(r));
      return kInvalid;
    }
  }
  const uint64_t span = (uint64_t)batch * 2 * level * c->n;
  if (spans_overlap(out, span, in, span)) {
    set_error("fhe_rotate_sum_hoisted: out must not overlap in");
    return kInvalid;
  }
  if ((rc = ensure_ws(c, rotate_sum_hoisted_workspace_bytes(c, batch), &ws, hs(s)))) return rc;
  return launch_rotate_sum_hoisted(c, out, in, galois_elts, rot_b, rot_a, pt, level, count, batch,
                                   ws, hs(s));
}

size_t fhe_rotate_sum_multi_workspace(const fhe_ctx* c, uint32_t count, uint32_t batch) {
  return c ? rotate_sum_multi_workspace_bytes(c, count, batch) : 0;
}

int fhe_rotate_sum_multi(const fhe_ctx* c, uint64_t* out, const uint64_t* const* cts,
                         const uint32_t* galois_elts, const uint64_t* const* rot_b,
                         const uint64_t* const* rot_a, uint32_t count, uint32_t batch, void* ws,
                         fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_rotate_sum_multi");
  if (rc) return rc;
  return fhe_rotate_sum_multi_level(c, out, cts, galois_elts, rot_b, rot_a, c->L, count, batch, ws,
                                    s);
}

int fhe_rotate_sum_multi_level(const fhe_ctx* c, uint64_t* out, const uint64_t* const* cts,
                               const uint32_t* galois_elts, const uint64_t* const* rot_b,
                               const uint64_t* const* rot_a, uint32_t level, uint32_t count,
                               uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_rotate_sum_multi_level");
  if (rc) return rc;
  if (count == 0 || count > kRotSumMax) {
    set_error("fhe_rotate_sum_multi: count must be 1..16");
    return kInvalid;
  }
  if (!galois_elts || !cts || ((!rot_b || !rot_a) && std::any_of(galois_elts, galois_elts + count,
                                                                  [](uint32_t g) { return g != 1; }))) {
    set_error("fhe_rotate_sum_multi: null Galois element, ciphertext or key array");
    return kInvalid;
  }
  const uint64_t span = (uint64_t)batch * 2 * level * c->n;
  for (uint32_t r = 0; r < count; ++r) {
    if (!cts[r] || (galois_elts[r] != 1 && (!rot_b[r] || !rot_a[r]))) {
      set_error("fhe_rotate_sum_multi: null ciphertext or key pointer for term " +
                std::to_string(r));
      return kInvalid;
    }
    if (spans_overlap(out, span, cts[r], span)) {
      set_error("fhe_rotate_sum_multi: out must not overlap an input ciphertext (term " +
                std::to_string(r) + ")");
      return kInvalid;
    }
  }
  if ((rc = ensure_ws(c, rotate_sum_multi_workspace_bytes(c, count, batch), &ws, hs(s)))) return rc;
  return launch_rotate_sum_multi(c, out, cts, galois_elts, rot_b, rot_a, level, count, batch, ws,
                                 hs(s));
}

size_t fhe_linear_transform_workspace(const fhe_ctx* c, uint32_t n2, uint32_t batch) {
  return c ? linear_transform_workspace_bytes(c, n2, batch) : 0;
}

int fhe_linear_transform(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t n1,
                         uint32_t n2, const uint32_t* baby_elts, const uint64_t* const* baby_b,
                         const uint64_t* const* baby_a, const uint32_t* giant_elts,
                         const uint64_t* const* giant_b, const uint64_t* const* giant_a,
                         const uint64_t* const* pt, uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_linear_transform");
  if (rc) return rc;
  return fhe_linear_transform_level(c, out, in, n1, n2, baby_elts, baby_b, baby_a, giant_elts,
                                    giant_b, giant_a, pt, c->L, batch, ws, s);
}

int fhe_linear_transform_level(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t n1,
                               uint32_t n2, const uint32_t* baby_elts,
                               const uint64_t* const* baby_b, const uint64_t* const* baby_a,
                               const uint32_t* giant_elts, const uint64_t* const* giant_b,
                               const uint64_t* const* giant_a, const uint64_t* const* pt,
                               uint32_t level, uint32_t batch, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_linear_transform_level");
  if (rc) return rc;
  if (n1 == 0 || n1 > kRotSumMax || n2 == 0 || n2 > kRotSumMax) {
    set_error("fhe_linear_transform: n1 and n2 must be 1..16");
    return kInvalid;
  }
  if (!baby_elts || !giant_elts || !pt) {
    set_error("fhe_linear_transform: null Galois element or plaintext array");
    return kInvalid;
  }
  auto keyed = [](const uint32_t* e, uint32_t k, const uint64_t* const* b, const uint64_t* const* a) {
    for (uint32_t r = 0; r < k; ++r)
      if (e[r] != 1 && (!b || !a || !b[r] || !a[r])) return false;
    return true;
  };
  if (!keyed(baby_elts, n1, baby_b, baby_a) || !keyed(giant_elts, n2, giant_b, giant_a)) {
    set_error("fhe_linear_transform: a rotated baby or giant step without its key");
    return kInvalid;
  }
  for (uint64_t r = 0; r < (uint64_t)n1 * n2; ++r)
    if (!pt[r]) {
      set_error("fhe_linear_transform: null plaintext pointer " + std::to_string(r));
      return kInvalid;
    }
  const uint64_t span = (uint64_t)batch * 2 * level * c->n;
  if (spans_overlap(out, span, in, span)) {
    set_error("fhe_linear_transform: out must not overlap in");
    return kInvalid;
  }
  if ((rc = ensure_ws(c, linear_transform_workspace_bytes(c, n2, batch), &ws, hs(s)))) return rc;
  return launch_linear_transform(c, out, in, n1, n2, baby_elts, baby_b, baby_a, giant_elts, giant_b,
                                 giant_a, pt, level, batch, ws, hs(s));
}

size_t fhe_mul_relin_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? mul_relin_workspace_bytes(c, batch) : 0;
}

int fhe_mul_relin(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                  const uint64_t* evk_b, const uint64_t* evk_a, uint32_t batch, int rescale,
                  void* ws, fhe_stream_t s) {
  int rc = check_window(c, 0, c ? c->L : 0, c ? c->L : 0, "fhe_mul_relin");
  if (rc) return rc;
  return fhe_mul_relin_level(c, out, a, b, evk_b, evk_a, c->L, batch, rescale, ws, s);
}

int fhe_mul_relin_level(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                        const uint64_t* evk_b, const uint64_t* evk_a, uint32_t level,
                        uint32_t batch, int rescale, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_mul_relin_level");
  if (rc) return rc;
  if (rescale && level < 2) {
    set_error("fhe_mul_relin_level: rescale needs level >= 2");
    return kInvalid;
  }
  if ((rc = ensure_ws(c, mul_relin_workspace_bytes(c, ks_pass_batch(c, batch)), &ws, hs(s)))) return rc;
  return launch_mul_relin(c, out, a, b, evk_b, evk_a, level, batch, rescale != 0, ws, hs(s));
}

int fhe_mul_sum_relin_level(const fhe_ctx* c, uint64_t* out, const uint64_t* const* a,
                            const uint32_t* a_levels, const uint64_t* const* b,
                            const uint32_t* b_levels, const uint64_t* evk_b, const uint64_t* evk_a,
                            uint32_t level, uint32_t count, uint32_t batch, int rescale, void* ws,
                            fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_mul_sum_relin_level");
  if (rc) return rc;
  if (c->K == 0) {
    set_error("fhe_mul_sum_relin_level: context has no special primes (K = 0)");
    return kInvalid;
  }
  if (count == 0 || count > kMulSumMax) {
    set_error("fhe_mul_sum_relin_level: count must be 1..16");
    return kInvalid;
  }
  if (rescale && level < 2) {
    set_error("fhe_mul_sum_relin_level: rescale needs level >= 2");
    return kInvalid;
  }
  if (!out || !a || !a_levels || !b || !b_levels || !evk_b || !evk_a) {
    set_error("fhe_mul_sum_relin_level: null output, ciphertext array, level array or key");
    return kInvalid;
  }
  const uint64_t out_words = (uint64_t)batch * 2 * (level - (rescale ? 1 : 0)) * c->n;
  for (uint32_t t = 0; t < count; ++t) {
    if (!a[t] || !b[t]) {
      set_error("fhe_mul_sum_relin_level: null ciphertext pointer in term " + std::to_string(t));
      return kInvalid;
    }
    if (a_levels[t] < level || a_levels[t] > c->L || b_levels[t] < level || b_levels[t] > c->L) {
      set_error("fhe_mul_sum_relin_level: the levels of term " + std::to_string(t) +
                " must be in [level, L]");
      return kInvalid;
    }
    if (spans_overlap(out, out_words, a[t], (uint64_t)batch * 2 * a_levels[t] * c->n) ||
        spans_overlap(out, out_words, b[t], (uint64_t)batch * 2 * b_levels[t] * c->n)) {
      set_error("fhe_mul_sum_relin_level: out overlaps an input of term " + std::to_string(t));
      return kInvalid;
    }
  }
  if (batch == 0) return kOk;
  if ((rc = ensure_ws(c, mul_relin_workspace_bytes(c, ks_pass_batch(c, batch)), &ws, hs(s)))) return rc;
  return launch_mul_sum_relin(c, out, a, a_levels, b, b_levels, evk_b, evk_a, level, count, batch,
                              rescale != 0, ws, hs(s));
}

size_t fhe_lincomb_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? lincomb_workspace_bytes(c, batch) : 0;
}

// out [batch][2][out_level][N] against one input of in_words words: the input itself, in place
// (same start, same stride, no rescale), or disjoint from it
static int check_plain_alias(const uint64_t* out, uint64_t out_words, const uint64_t* in,
                             uint64_t in_words, bool in_place_ok, const std::string& what) {
  if (in_place_ok && out == in && out_words == in_words) return kOk;
  if (spans_overlap(out, out_words, in, in_words)) {
    set_error(what + " (out is either that input itself -- same start, same level, no rescale "
                     "-- or disjoint from it)");
    return kInvalid;
  }
  return kOk;
}

int fhe_lincomb_level(const fhe_ctx* c, uint64_t* out, const uint64_t* const* cts,
                      const uint32_t* in_levels, const uint64_t* scalars, uint32_t scalar_stride,
                      int has_const, uint32_t level, uint32_t count, uint32_t batch, int rescale,
                      void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_lincomb_level");
  if (rc) return rc;
  if (count == 0 || count > kLincombMax) {
    set_error("fhe_lincomb_level: count must be 1..16");
    return kInvalid;
  }
  if (rescale && level < 2) {
    set_error("fhe_lincomb_level: rescale needs level >= 2");
    return kInvalid;
  }
  if (scalar_stride < level) {
    set_error("fhe_lincomb_level: scalar_stride must be at least level");
    return kInvalid;
  }
  if (!out || !cts || !in_levels || !scalars) {
    set_error("fhe_lincomb_level: null output, ciphertext array, level array or scalar table");
    return kInvalid;
  }
  const uint64_t out_words = (uint64_t)batch * 2 * (level - (rescale ? 1 : 0)) * c->n;
  for (uint32_t t = 0; t < count; ++t) {
    if (!cts[t]) {
      set_error("fhe_lincomb_level: null ciphertext pointer for term " + std::to_string(t));
      return kInvalid;
    }
    if (in_levels[t] < level || in_levels[t] > c->L) {
      set_error("fhe_lincomb_level: in_levels[" + std::to_string(t) + "] must be in [level, L]");
      return kInvalid;
    }
    if ((rc = check_plain_alias(out, out_words, cts[t], (uint64_t)batch * 2 * in_levels[t] * c->n,
                                !rescale, "fhe_lincomb_level: out overlaps term " +
                                              std::to_string(t))))
      return rc;
  }
  if (batch == 0) return kOk;
  if (rescale && (rc = ensure_ws(c, lincomb_workspace_bytes(c, batch), &ws, hs(s)))) return rc;
  return launch_lincomb(c, out, cts, in_levels, scalars, scalar_stride, has_const != 0, level,
                        count, batch, rescale != 0, ws, hs(s));
}

int fhe_mul_plain_level(const fhe_ctx* c, uint64_t* out, const uint64_t* ct, const uint64_t* pt,
                        uint32_t pt_rows, uint32_t pt_batch, uint32_t level, uint32_t batch,
                        int rescale, void* ws, fhe_stream_t s) {
  int rc = check_level(c, level, "fhe_mul_plain_level");
  if (rc) return rc;
  if (rescale && level < 2) {
    set_error("fhe_mul_plain_level: rescale needs level >= 2");
    return kInvalid;
  }
  if (pt_rows < level) {
    set_error("fhe_mul_plain_level: pt_rows must be at least level");
    return kInvalid;
  }
  if (pt_batch != 1 && pt_batch != batch) {
    set_error("fhe_mul_plain_level: pt_batch must be 1 or batch");
    return kInvalid;
  }
  if (!out || !ct || !pt) {
    set_error("fhe_mul_plain_level: null data pointer");
    return kInvalid;
  }
  const uint64_t ct_words = (uint64_t)batch * 2 * level * c->n;
  const uint64_t out_words = (uint64_t)batch * 2 * (level - (rescale ? 1 : 0)) * c->n;
  if ((rc = check_plain_alias(out, out_words, ct, ct_words, !rescale,
                              "fhe_mul_plain_level: out overlaps ct")) ||
      (rc = check_plain_alias(out, out_words, pt, (uint64_t)pt_batch * pt_rows * c->n, false,
                              "fhe_mul_plain_level: out overlaps pt")))
    return rc;
  if (batch == 0) return kOk;
  if (rescale && (rc = ensure_ws(c, lincomb_workspace_bytes(c, batch), &ws, hs(s)))) return rc;
  return launch_mul_plain(c, out, ct, pt, pt_rows, pt_batch, level, batch, rescale != 0, ws, hs(s));
}

// the shared checks of fhe_conj_split_level / fhe_conj_merge_level: outs[] against ins[], all
// [batch][2][level][N]
static int conj_check(const fhe_ctx* c, uint64_t* const* outs, int nout, const uint64_t* const* ins,
                      uint32_t level, uint32_t batch, const char* who) {
  int rc = check_level(c, level, who);
  if (rc) return rc;
  for (int i = 0; i < nout; ++i)
    if (!outs[i]) return (set_error(std::string(who) + ": null data pointer"), kInvalid);
  if (!ins[0] || !ins[1]) return (set_error(std::string(who) + ": null data pointer"), kInvalid);
  const uint64_t words = (uint64_t)batch * 2 * level * c->n;
  for (int i = 0; i < nout; ++i)
    for (int j = 0; j < 2; ++j)
      if ((rc = check_plain_alias(outs[i], words, ins[j], words, true,
                                  std::string(who) + ": an output overlaps an input")))
        return rc;
  if (nout == 2 && spans_overlap(outs[0], words, outs[1], words)) {
    set_error(std::string(who) + ": re and im overlap");
    return kInvalid;
  }
  return kOk;
}

int fhe_conj_split_level(const fhe_ctx* c, uint64_t* re, uint64_t* im, const uint64_t* ct,
                         const uint64_t* cc, uint32_t level, uint32_t batch, fhe_stream_t s) {
  uint64_t* outs[2] = {re, im};
  const uint64_t* ins[2] = {ct, cc};
  if (int rc = conj_check(c, outs, 2, ins, level, batch, "fhe_conj_split_level")) return rc;
  return launch_conj(c, false, re, im, ct, cc, level, batch, hs(s));
}

int fhe_conj_merge_level(const fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b,
                         uint32_t level, uint32_t batch, fhe_stream_t s) {
  uint64_t* outs[1] = {out};
  const uint64_t* ins[2] = {a, b};
  if (int rc = conj_check(c, outs, 1, ins, level, batch, "fhe_conj_merge_level")) return rc;
  return launch_conj(c, true, out, nullptr, a, b, level, batch, hs(s));
}

size_t fhe_mod_raise_workspace(const fhe_ctx* c, uint32_t batch) {
  return c ? mod_raise_workspace_bytes(c, batch) : 0;
}

int fhe_mod_raise(const fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t in_level,
                  uint32_t out_level, uint32_t batch, void* ws, fhe_stream_t s) {
  if (!c) {
    set_error("fhe_mod_raise: null context");
    return kInvalid;
  }
  if (in_level == 0 || in_level > c->L || out_level == 0 || out_level > c->L) {
    set_error("fhe_mod_raise: in_level and out_level must be in [1, L]");
    return kInvalid;
  }
  if (!out || !in) {
    set_error("fhe_mod_raise: null data pointer");
    return kInvalid;
  }
  if (spans_overlap(out, (uint64_t)batch * 2 * out_level * c->n, in,
                    (uint64_t)batch * 2 * in_level * c->n)) {
    set_error("fhe_mod_raise: out overlaps in");
    return kInvalid;
  }
  if (batch == 0) return kOk;
  int rc = ensure_ws(c, mod_raise_workspace_bytes(c, batch), &ws, hs(s));
  if (rc) return rc;
  // FHECORE_MODRAISE_UNFUSED=1: the separate-spread form of wide contexts on any context (the
  // same bits; tools/modraise_times.py times the two against each other)
  const char* u = std::getenv("FHECORE_MODRAISE_UNFUSED");
  return launch_mod_raise(c, out, in, in_level, out_level, batch, ws, u && u[0] == '1', hs(s));
}

size_t fhe_encode_workspace(const fhe_ctx* c, uint32_t count) {
  return c ? encode_workspace_bytes(c, count) : 0;
}

int fhe_encode_roots(uint32_t log_n, double* out) {
  if (log_n < 10 || log_n > 17) {
    set_error("fhe_encode_roots: log_n must be in [10, 17]");
    return kUnsupported;
  }
  if (!out) {
    set_error("fhe_encode_roots: null output");
    return kInvalid;
  }
  encode_roots(log_n, out);
  return kOk;
}

// fhe_encode and fhe_encode_sparse (log_slots < 0: full packing, log_n - 1)
static int encode_call(const char* who, const fhe_ctx* c, uint64_t* out, const double* slots,
                       double delta, int64_t log_slots, uint32_t level, int special,
                       uint32_t count, void* ws, fhe_stream_t s) {
  const std::string w(who);
  // (the scale first: it needs no context, so a CPU-only machine can check the refusal)
  if (!(std::isfinite(delta) && delta > 0)) {
    set_error(w + ": delta must be finite and positive");
    return kInvalid;
  }
  if (!c) {
    set_error(w + ": null context");
    return kInvalid;
  }
  if (log_slots < 0) log_slots = c->log_n - 1;
  if (log_slots > (int64_t)c->log_n - 1) {
    set_error(w + ": log_slots must be in [0, log_n - 1]");
    return kInvalid;
  }
  if (level == 0 || level > c->L) {
    set_error(w + ": level must be in [1, L]");
    return kInvalid;
  }
  if (special && c->K == 0) {
    set_error(w + ": special needs a context with P-limbs (K > 0)");
    return kInvalid;
  }
  if (!out || !slots) {
    set_error(w + ": null data pointer");
    return kInvalid;
  }
  const uint64_t rows = level + (special ? c->K : 0);
  if (spans_overlap(out, (uint64_t)count * rows * c->n, reinterpret_cast<const uint64_t*>(slots),
                    (uint64_t)count << (log_slots + 1))) {
    set_error(w + ": out overlaps slots");
    return kInvalid;
  }
  if (count == 0) return kOk;
  int rc = ensure_ws(c, encode_workspace_bytes(c, count), &ws, hs(s));
  if (rc) return rc;
  // FHECORE_ENCODE_UNFUSED=1: the separate-spread form of wide contexts on any context (the same
  // bits; tools/encode_times.py times the two against each other)
  const char* u = std::getenv("FHECORE_ENCODE_UNFUSED");
  return launch_encode(c, out, slots, delta, (uint32_t)log_slots, level, special != 0, count, ws,
                       u && u[0] == '1', hs(s));
}

int fhe_encode(const fhe_ctx* c, uint64_t* out, const double* slots, double delta, uint32_t level,
               int special, uint32_t count, void* ws, fhe_stream_t s) {
  return encode_call("fhe_encode", c, out, slots, delta, -1, level, special, count, ws, s);
}

int fhe_encode_sparse(const fhe_ctx* c, uint64_t* out, const double* slots, double delta,
                      uint32_t log_slots, uint32_t level, int special, uint32_t count, void* ws,
                      fhe_stream_t s) {
  return encode_call("fhe_encode_sparse", c, out, slots, delta, log_slots, level, special, count,
                     ws, s);
}

size_t fhe_decode_workspace(const fhe_ctx* c, uint32_t count) {
  return c ? decode_workspace_bytes(c, count) : 0;
}

static int decode_call(const char* who, const fhe_ctx* c, double* slots, const uint64_t* pt,
                       double delta, int64_t log_slots, uint32_t pt_rows, uint32_t level,
                       uint32_t count, void* ws, fhe_stream_t s) {
  const std::string w(who);
  // (the scale first: it needs no context, so a CPU-only machine can check the refusal)
  if (!(std::isfinite(delta) && delta > 0)) {
    set_error(w + ": delta must be finite and positive");
    return kInvalid;
  }
  if (!c) {
    set_error(w + ": null context");
    return kInvalid;
  }
  if (log_slots < 0) log_slots = c->log_n - 1;
  if (log_slots > (int64_t)c->log_n - 1) {
    set_error(w + ": log_slots must be in [0, log_n - 1]");
    return kInvalid;
  }
  if (level == 0 || level > c->L) {
    set_error(w + ": level must be in [1, L]");
    return kInvalid;
  }
  if (pt_rows < std::min<uint32_t>(level, 2)) {
    set_error(w + ": pt_rows must cover the limbs read (min(level, 2))");
    return kInvalid;
  }
  if (!slots || !pt) {
    set_error(w + ": null data pointer");
    return kInvalid;
  }
  if (spans_overlap(reinterpret_cast<const uint64_t*>(slots), (uint64_t)count << (log_slots + 1),
                    pt, (uint64_t)count * pt_rows * c->n)) {
    set_error(w + ": slots overlaps pt");
    return kInvalid;
  }
  if (count == 0) return kOk;
  int rc = ensure_ws(c, decode_workspace_bytes(c, count), &ws, hs(s));
  if (rc) return rc;
  return launch_decode(c, slots, pt, delta, (uint32_t)log_slots, pt_rows, level, count, ws, hs(s));
}

int fhe_decode(const fhe_ctx* c, double* slots, const uint64_t* pt, double delta, uint32_t pt_rows,
               uint32_t level, uint32_t count, void* ws, fhe_stream_t s) {
  return decode_call("fhe_decode", c, slots, pt, delta, -1, pt_rows, level, count, ws, s);
}

int fhe_decode_sparse(const fhe_ctx* c, double* slots, const uint64_t* pt, double delta,
                      uint32_t log_slots, uint32_t pt_rows, uint32_t level, uint32_t count,
                      void* ws, fhe_stream_t s) {
  return decode_call("fhe_decode_sparse", c, slots, pt, delta, log_slots, pt_rows, level, count,
                     ws, s);
}

int fhe_decrypt_slots(const fhe_ctx* c, double* slots, const uint64_t* ct, const uint64_t* sk,
                      double delta, uint32_t log_slots, uint32_t level, uint32_t batch, void* ws,
                      fhe_stream_t s) {
  const std::string w("fhe_decrypt_slots");
  if (!c) {
    set_error(w + ": null context");
    return kInvalid;
  }
  if (!slots || !ct || !sk) {
    set_error(w + ": null data pointer");
    return kInvalid;
  }
  if (level == 0 || level > c->L) {
    set_error(w + ": level must be in [1, L]");
    return kInvalid;
  }
  if (log_slots > c->log_n - 1) {
    set_error(w + ": log_slots must be in [0, log_n - 1]");
    return kInvalid;
  }
  if (!(std::isfinite(delta) && delta > 0)) {
    set_error(w + ": delta must be finite and positive");
    return kInvalid;
  }
  const uint64_t n = c->n;
  const uint64_t* sw = reinterpret_cast<const uint64_t*>(slots);
  const uint64_t slot_words = (uint64_t)batch << (log_slots + 1);
  if (spans_overlap(sw, slot_words, ct, (uint64_t)batch * 2 * level * n)) {
    set_error(w + ": slots overlaps ct");
    return kInvalid;
  }
  if (spans_overlap(sw, slot_words, sk, std::min<uint64_t>(level, 2) * n)) {
    set_error(w + ": slots overlaps sk");
    return kInvalid;
  }
  const size_t ws_bytes = decode_workspace_bytes(c, batch);
  if (ws && spans_overlap(sw, slot_words, static_cast<const uint64_t*>(ws), ws_bytes / 8)) {
    set_error(w + ": slots overlaps the workspace");
    return kInvalid;
  }
  if (batch == 0) return kOk;
  int rc = ensure_ws(c, ws_bytes, &ws, hs(s));
  if (rc) return rc;
  // FHECORE_DECRYPT_UNFUSED=1: the form of wide contexts (the product written out, then the whole
  // inverse transform) on any context (the same bits; tools/decrypt_times.py times the two)
  const char* u = std::getenv("FHECORE_DECRYPT_UNFUSED");
  return launch_decrypt_slots(c, slots, ct, sk, delta, log_slots, level, batch, ws,
                              u && u[0] == '1', hs(s));
}

size_t fhe_encrypt_workspace(const fhe_ctx* c, uint32_t level, uint32_t batch) {
  return c && level >= 1 && level <= c->L ? encrypt_workspace_bytes(c, level, batch) : 0;
}

// fhe_encrypt_level, fhe_encrypt_sk_level and fhe_encrypt_slots: a.ct, a.key, a.level, a.batch and
// either (pt, pt_rows, pt_batch) or (slots, delta, log_slots) as the caller gave them
static int encrypt_call(const char* who, const fhe_ctx* c, EncryptArgs a, bool slots_form,
                        uint64_t index0, void* ws, fhe_stream_t s) {
  const std::string w(who);
  if (!c) {
    set_error(w + ": null context");
    return kInvalid;
  }
  if (!a.ct || !a.key) {
    set_error(w + ": null ciphertext or key");
    return kInvalid;
  }
  if (a.level == 0 || a.level > c->L) {
    set_error(w + ": level must be in [1, L]");
    return kInvalid;
  }
  if (index0 + a.batch > (1ull << 32)) {
    set_error(w + ": index0 + batch exceeds 2^32 (the Philox counter's poly field)");
    return kInvalid;
  }
  const uint64_t n = c->n;
  const uint64_t ct_words = (uint64_t)a.batch * 2 * a.level * n;
  if (slots_form) {
    if (!a.slots) {
      set_error(w + ": null slots");
      return kInvalid;
    }
    if (!(std::isfinite(a.delta) && a.delta > 0)) {
      set_error(w + ": delta must be finite and positive");
      return kInvalid;
    }
    if (a.log_slots > c->log_n - 1) {
      set_error(w + ": log_slots must be in [0, log_n - 1]");
      return kInvalid;
    }
    if (spans_overlap(a.ct, ct_words, reinterpret_cast<const uint64_t*>(a.slots),
                      (uint64_t)a.batch << (a.log_slots + 1))) {
      set_error(w + ": ct overlaps slots");
      return kInvalid;
    }
  } else {
    if (a.pt_batch != 1 && a.pt_batch != a.batch) {
      set_error(w + ": pt_batch must be 1 or batch");
      return kInvalid;
    }
    if (a.pt && a.pt_rows < a.level) {
      set_error(w + ": pt_rows must be at least level");
      return kInvalid;
    }
    if (a.pt && spans_overlap(a.ct, ct_words, a.pt, (uint64_t)a.pt_batch * a.pt_rows * n)) {
      set_error(w + ": ct overlaps pt");
      return kInvalid;
    }
  }
  if (spans_overlap(a.ct, ct_words, a.key, (a.secret ? c->L + c->K : 2 * (uint64_t)c->L) * n)) {
    set_error(w + ": ct overlaps the key");
    return kInvalid;
  }
  const size_t ws_bytes = encrypt_workspace_bytes(c, a.level, a.batch);
  if (ws && spans_overlap(a.ct, ct_words, static_cast<const uint64_t*>(ws), ws_bytes / 8)) {
    set_error(w + ": ct overlaps the workspace");
    return kInvalid;
  }
  if (a.batch == 0) return kOk;
  a.index0 = (uint32_t)index0;
  int rc = ensure_ws(c, ws_bytes, &ws, hs(s));
  if (rc) return rc;
  // FHECORE_ENCRYPT_UNFUSED=1: the spread-and-whole-NTT form of wide contexts on any context;
  // FHECORE_ENCRYPT_PASS=p: at most p ciphertexts per pass.  The same bits either way
  // (tools/encrypt_times.py times them against the defaults)
  const char* u = std::getenv("FHECORE_ENCRYPT_UNFUSED");
  const char* p = std::getenv("FHECORE_ENCRYPT_PASS");
  const long pass = p ? std::atol(p) : 0;
  return launch_encrypt(c, a, ws, u && u[0] == '1', pass > 0 ? (uint32_t)std::min(pass, 1L << 30) : 0,
                        hs(s));
}

int fhe_encrypt_level(const fhe_ctx* c, uint64_t* ct, const uint64_t* pt, uint32_t pt_rows,
                      uint32_t pt_batch, const uint64_t* pk, uint32_t level, uint32_t batch,
                      uint64_t seed, uint32_t index0, void* ws, fhe_stream_t s) {
  EncryptArgs a{ct, pt, pt_rows, pt_batch, nullptr, 0.0, 0, pk, false, level, batch, seed, 0};
  return encrypt_call("fhe_encrypt_level", c, a, false, index0, ws, s);
}

int fhe_encrypt_sk_level(const fhe_ctx* c, uint64_t* ct, const uint64_t* pt, uint32_t pt_rows,
                         uint32_t pt_batch, const uint64_t* sk, uint32_t level, uint32_t batch,
                         uint64_t seed, uint32_t index0, void* ws, fhe_stream_t s) {
  EncryptArgs a{ct, pt, pt_rows, pt_batch, nullptr, 0.0, 0, sk, true, level, batch, seed, 0};
  return encrypt_call("fhe_encrypt_sk_level", c, a, false, index0, ws, s);
}

int fhe_encrypt_slots(const fhe_ctx* c, uint64_t* ct, const double* slots, double delta,
                      uint32_t log_slots, const uint64_t* key, int secret_key, uint32_t level,
                      uint32_t batch, uint64_t seed, uint32_t index0, void* ws, fhe_stream_t s) {
  EncryptArgs a{ct,  nullptr,         0,     1,     slots, delta, log_slots,
                key, secret_key != 0, level, batch, seed,  0};
  return encrypt_call("fhe_encrypt_slots", c, a, true, index0, ws, s);
}

}  // extern "C"
