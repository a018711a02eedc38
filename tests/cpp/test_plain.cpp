// C++ API for the plaintext arithmetic (run by tests/test_cpp_programs.py on a GPU box):
// Evaluator::lincomb (mixed levels, constant, rescale), mul_plain and drop_level compared word for
// word with the C entry points (fhe_lincomb_level, fhe_mul_plain_level) and, for drop_level, with
// the sliced host array.
#include <cstdio>
#include <random>

#include "fhecore.hpp"

using u64 = uint64_t;

static bool same_words(const fhe::DeviceBuffer& a, const fhe::DeviceBuffer& b, size_t words) {
  const std::vector<u64> x = a.download(), y = b.download();
  if (x.size() < words || y.size() < words) return false;
  for (size_t i = 0; i < words; ++i)
    if (x[i] != y[i]) return false;
  return true;
}

int main() {
  try {
    const uint32_t log_n = 10, L = 4;
    fhe::Context kc = fhe::Context::standard(log_n, L, 2, 2);
    const u64 n = kc.n();
    fhe::Evaluator ev(kc);
    std::vector<u64> q(L + 2);
    fhe::check(fhe_ctx_moduli(kc.get(), q.data(), nullptr), "moduli");
    std::mt19937_64 rng(11);
    auto random_ct = [&](uint32_t comps, uint32_t limbs) {
      std::vector<u64> h((size_t)comps * limbs * n);
      for (uint32_t c = 0; c < comps; ++c)
        for (uint32_t l = 0; l < limbs; ++l)
          for (u64 i = 0; i < n; ++i) h[((size_t)c * limbs + l) * n + i] = rng() % q[l];
      fhe::Ciphertext x(kc, comps, limbs, true);
      x.buf.upload(h);
      return x;
    };
    const fhe::Ciphertext a = random_ct(2, L), b = random_ct(2, L - 1), pt = random_ct(1, L);
    // scalars [3][L]: two terms and the constant
    std::vector<u64> hs(3 * L);
    for (uint32_t r = 0; r < 3; ++r)
      for (uint32_t l = 0; l < L; ++l) hs[r * L + l] = rng() % q[l];
    fhe::DeviceBuffer sc(3 * L);
    sc.upload(hs);

    // lincomb at the lower input's level (3), with the constant, with and without rescale
    const uint32_t lv = L - 1;
    const uint64_t* cts[2] = {a.data(), b.data()};
    const uint32_t in_levels[2] = {L, L - 1};
    for (int rescale = 0; rescale < 2; ++rescale) {
      const fhe::Ciphertext y = ev.lincomb({&a, &b}, sc, L, true, rescale != 0);
      const size_t words = (size_t)2 * (lv - rescale) * n;
      fhe::DeviceBuffer cy(words);
      fhe::check(fhe_lincomb_level(kc.get(), cy.data(), cts, in_levels, sc.data(), L, 1, lv, 2, 1,
                                   rescale, nullptr, nullptr),
                 "fhe_lincomb_level");
      fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
      if (y.limbs != lv - rescale || !same_words(y.buf, cy, words)) {
        std::printf("FAIL lincomb (rescale %d) differs from fhe_lincomb_level\n", rescale);
        return 1;
      }
    }
    // mul_plain with a top-level plaintext at level 3
    for (int rescale = 0; rescale < 2; ++rescale) {
      const fhe::Ciphertext y = ev.mul_plain(b, pt, rescale != 0);
      const size_t words = (size_t)2 * (lv - rescale) * n;
      fhe::DeviceBuffer cy(words);
      fhe::check(fhe_mul_plain_level(kc.get(), cy.data(), b.data(), pt.data(), L, 1, lv, 1, rescale,
                                     nullptr, nullptr),
                 "fhe_mul_plain_level");
      fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
      if (y.limbs != lv - rescale || !same_words(y.buf, cy, words)) {
        std::printf("FAIL mul_plain (rescale %d) differs from fhe_mul_plain_level\n", rescale);
        return 1;
      }
    }
    // drop_level: the first two limbs of each polynomial
    const fhe::Ciphertext d = ev.drop_level(a, 2);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    const std::vector<u64> ha = a.buf.download(), hd = d.buf.download();
    bool ok = d.limbs == 2 && hd.size() == (size_t)2 * 2 * n;
    for (uint32_t c = 0; ok && c < 2; ++c)
      for (uint32_t l = 0; ok && l < 2; ++l)
        for (u64 i = 0; i < n; ++i)
          if (hd[((size_t)c * 2 + l) * n + i] != ha[((size_t)c * L + l) * n + i]) {
            ok = false;
            break;
          }
    if (!ok) {
      std::printf("FAIL drop_level differs from the slice\n");
      return 1;
    }
    // rescale with one limb left is refused, at both layers
    const fhe::Ciphertext one = ev.drop_level(a, 1);
    bool threw = false;
    try {
      (void)ev.lincomb({&one}, sc, L, false, true);
    } catch (const fhe::Error&) {
      threw = true;
    }
    fhe::DeviceBuffer c0((size_t)2 * n);
    const uint64_t* c1[1] = {one.data()};
    const uint32_t l1[1] = {1};
    if (!threw || fhe_lincomb_level(kc.get(), c0.data(), c1, l1, sc.data(), L, 0, 1, 1, 1, 1, nullptr,
                                    nullptr) != FHE_EINVAL) {
      std::printf("FAIL rescale at one limb was not refused\n");
      return 1;
    }
    std::printf("cpp plain ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
