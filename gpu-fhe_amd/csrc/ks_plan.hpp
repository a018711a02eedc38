// The hybrid key-switch's host-side plan: which kernels a call takes and where its workspace
// regions lie, decided once.  Pure host code without HIP (tests/cpp/host_sanitize.cpp sweeps it);
// internal.hpp fills KsShape from fhe_ctx, rns.hip launch_keyswitch_shard executes the plan and
// every caller that must agree with it (the INTT feeding it, the epilogue's addend, a composite
// workspace) reads the same struct.  DESIGN.md "Key-switch" tabulates the flags.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace fhe {

// What the decisions read of a context (fhe_ctx's fields of the same names).
struct KsShape {
  uint32_t L, K, dnum, alpha;
  uint64_t n;
  bool wide, lz16;
};

enum KsMode : int {
  kKsFull = 0,     // ModUp, inner product, ModDown
  kKsModUpOnly,    // a hoisted rotation's shared ModUp: the NTT-form digits stay in `ext`
  kKsHoistInner,   // a hoisted rotation's own step: gathered inner product over `ext`, ModDown
  kKsAccReady,     // the caller has filled `acc` itself (the rotation sums): ModDown only
};

struct KsPlan {
  // the call: this rank's Q-limbs [limb0, limb0 + nlimbs) of `batch` ciphertexts; level != 0: the
  // chain's first `level` Q-limbs (then limb0 = 0, nlimbs = level), the top-level key read in place
  uint32_t limb0, nlimbs, batch, level;
  KsMode mode;
  // The chain's live Q-limbs (all L, or a level call's first `level`) in ceil(liveq / alpha)
  // digits of the top-level width alpha: an empty last digit (dnum alpha - alpha >= L) is never
  // live, and the last live one is partial where alpha does not divide a level below the top
  // (its constants: fhe_ctx's d_lvl_* tables).  rows = nlimbs + K extended rows per digit;
  // key_rows: rows of one digit of the key as stored (a level call reads rows
  // {0 .. level-1} u {L .. L+K-1} of the top-level key in place).
  uint32_t liveq, digits, rows, key_rows, alpha;
  bool partial;

  // Path flags (what selects each and the kernel it implies: DESIGN.md "Key-switch").
  // fused: the digits get only their column-forward pass and k_ks_row_inner runs every digit's
  // row-forward pass and the inner product (no NTT-form ext in HBM); else full NTTs + k_ks_inner.
  // Wide contexts (a modulus >= 2^61) take the unfused kernels: the fused ones rely on lazy ranges
  // and 128-bit sums that need q < 2^61.  So do the hoisted modes: the digits must exist in NTT
  // form in HBM so that each rotation's inner product can gather them through its automorphism.
  bool fused;
  // the hoisted ModUp on the contexts the fused ModUp serves: the same conversion column pass
  // (plain table: the gathered inner products read plain residues), then one row-forward pass per
  // digit range, in place of k_baseconv + a full NTT per range
  bool hoist_up;
  // the base conversion runs inside the column-forward pass (k_modup_col) after a one-pass
  // prologue that scales the digit's source rows (digits of <= 4 limbs); the extended rows are
  // never written in coefficient form
  bool fused_up;
  // lz16 fused ModUp: the extended rows come out times R = 2^64 (d_modup_hat_rw / _rwp), which
  // k_ks_row_inner's Montgomery inner product cancels (KsRowArgs::mont)
  bool mont_ext;
  // ModDown's P -> Q conversion runs inside the conversion NTT's column-forward pass
  // (k_modup_col) and k_moddown_row finishes; a hoisted step takes it with a scratch of its own
  // for the INTT output (the ext region is taken)
  bool fused_down;
  // ModDown's P^-1 folded into the accumulators' Q rows (the ModUp conversion tables of the Q
  // targets and the own digit's R factor carry P^-1) and into the P -> Q conversion table, so
  // the finish is a subtraction
  bool pscale;
  // k_ks_row_inner also runs the first (row) pass of ModDown's INTT on the special rows
  bool row_pinv;
  // With P^-1 in the constants the Q rows wait for ModDown's conversion and finish in the same
  // workgroup (k_ks_row_fin): the row kernel covers only the special rows first, their column
  // inverse runs in place in the accumulators, and neither the accumulators' Q rows nor
  // k_moddown_row's pass over them touch HBM
  bool qfin;
  // the finish is k_moddown_row or k_ks_row_fin, which can gather the epilogue's addend through
  // an automorphism (KsEpilogue::add_gal); k_moddown_finish adds its addend rows un-permuted
  bool row_finish;
  // The input the fused ModUp can read "prepared": every Q-limb already scaled by (D^_k)^-1 of
  // its digit by the INTT that made it (d_nfold_up); a property of the context, every mode
  bool prepared;
  // the fused conversions' source format: lz16 contexts read plain residues, the others Sum30's
  // 30-bit pieces, which the INTTs and k_modup_scale feeding them emit directly
  bool split30;

  // Workspace regions, offsets in 64-bit words from the workspace's start, in this order:
  // ext [digits][batch][rows][N], acc [2][batch][rows][N], conv [2][batch][nlimbs][N],
  // yws [batch][alpha][N] (the fused ModUp's scaled sources), and at the tail c_all
  // [batch][liveq][N], where the single-device forms put INTT(d2)
  uint64_t ext, acc, conv, yws, call, total;

  // digit j < digits covers the live Q-limbs [lo(j), hi(j))
  uint32_t lo(uint32_t j) const { return j * alpha; }
  uint32_t hi(uint32_t j) const { return std::min(liveq, lo(j) + alpha); }
  // words of the digits region: a ModUp-only call writes nothing past it
  uint64_t ext_words() const { return acc - ext; }
  // words between the two accumulators
  uint64_t acc_stride() const { return (conv - acc) / 2; }
  uint64_t bytes() const { return total * sizeof(uint64_t); }
};

// ydn: a hoisted step was given the scratch its fused ModDown needs
inline KsPlan ks_plan(const KsShape& c, uint32_t limb0, uint32_t nlimbs, uint32_t batch,
                      uint32_t level, KsMode mode = kKsFull, bool ydn = false) {
  KsPlan p{};
  p.limb0 = limb0;
  p.nlimbs = nlimbs;
  p.batch = batch;
  p.level = level;
  p.mode = mode;
  p.alpha = c.alpha;
  p.liveq = level ? level : c.L;
  p.digits = c.alpha ? (p.liveq + c.alpha - 1) / c.alpha : 0;
  p.rows = nlimbs + c.K;
  p.key_rows = level ? c.L + c.K : p.rows;
  // (alpha = 0: a context without special primes, whose key-switch is refused; sizes only)
  p.partial = level && level < c.L && c.alpha && level % c.alpha != 0;

  const bool hoist = mode != kKsFull;
  const bool narrow4 = c.dnum <= 4 && !c.wide;
  p.prepared = c.K > 0 && narrow4 && c.alpha <= 4;
  p.split30 = !c.lz16;
  p.fused = !hoist && narrow4;
  p.hoist_up = mode == kKsModUpOnly && p.prepared;
  p.fused_up = (p.fused && c.alpha <= 4) || p.hoist_up;
  p.mont_ext = p.fused_up && !p.hoist_up && c.lz16;
  // (the fused form needs 2 K rows of ext free for the INTT's output)
  p.fused_down = c.K <= 4 && ((p.fused && (uint64_t)p.digits * p.rows >= 2 * (uint64_t)c.K) ||
                              (hoist && ydn && narrow4));
  p.pscale = p.mont_ext && p.fused_down;
  p.row_pinv = p.fused && p.fused_down;
  p.qfin = p.pscale && p.row_pinv;
  p.row_finish = p.fused || p.fused_down;

  const uint64_t bn = (uint64_t)batch * c.n;
  p.ext = 0;
  p.acc = p.ext + p.digits * bn * p.rows;
  p.conv = p.acc + 2 * bn * p.rows;
  p.yws = p.conv + 2 * bn * nlimbs;
  p.call = p.yws + bn * c.alpha;
  p.total = p.call + bn * p.liveq;
  return p;
}

}  // namespace fhe
