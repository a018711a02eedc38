// C++ API for the sum of products with one relinearisation (run by tests/test_cpp_programs.py on a
// GPU box): Evaluator::mul_sum_relin (mixed levels, a square, a shared operand, with and without
// rescale) compared word for word with the C entry point fhe_mul_sum_relin_level, and one term
// compared with Evaluator::mul_relin.
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
    fhe::KeyGenerator kg(kc, 42);
    const fhe::SwitchKey rl = kg.relin_key(46);
    fhe::Evaluator ev(kc);
    std::vector<u64> q(L + 2);
    fhe::check(fhe_ctx_moduli(kc.get(), q.data(), nullptr), "moduli");
    std::mt19937_64 rng(13);
    auto random_ct = [&](uint32_t limbs) {
      std::vector<u64> h((size_t)2 * limbs * n);
      for (uint32_t c = 0; c < 2; ++c)
        for (uint32_t l = 0; l < limbs; ++l)
          for (u64 i = 0; i < n; ++i) h[((size_t)c * limbs + l) * n + i] = rng() % q[l];
      fhe::Ciphertext x(kc, 2, limbs, true);
      x.buf.upload(h);
      return x;
    };
    const fhe::Ciphertext x = random_ct(L), y = random_ct(L - 1), z = random_ct(L);

    // three terms at the lowest level (3): x y, z z (a square), x z (x shared)
    const uint32_t lv = L - 1;
    const uint64_t* pa[3] = {x.data(), z.data(), x.data()};
    const uint64_t* pb[3] = {y.data(), z.data(), z.data()};
    const uint32_t la[3] = {L, L, L}, lb[3] = {L - 1, L, L};
    for (int rescale = 0; rescale < 2; ++rescale) {
      const fhe::Ciphertext r = ev.mul_sum_relin({&x, &z, &x}, {&y, &z, &z}, rl, rescale != 0);
      const size_t words = (size_t)2 * (lv - rescale) * n;
      fhe::DeviceBuffer cr(words);
      fhe::check(fhe_mul_sum_relin_level(kc.get(), cr.data(), pa, la, pb, lb, rl.b(), rl.a(), lv, 3, 1,
                                         rescale, nullptr, nullptr),
                 "fhe_mul_sum_relin_level");
      fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
      if (r.limbs != lv - rescale || !same_words(r.buf, cr, words)) {
        std::printf("FAIL mul_sum_relin (rescale %d) differs from fhe_mul_sum_relin_level\n", rescale);
        return 1;
      }
    }
    // an explicit level below the operands'
    {
      const fhe::Ciphertext r = ev.mul_sum_relin({&x, &z}, {&z, &z}, rl, true, 2);
      const uint32_t l2[2] = {L, L};
      fhe::DeviceBuffer cr((size_t)2 * n);
      fhe::check(fhe_mul_sum_relin_level(kc.get(), cr.data(), pa + 1, l2, pb + 1, l2, rl.b(), rl.a(), 2,
                                         2, 1, 1, nullptr, nullptr),
                 "fhe_mul_sum_relin_level");
      // (terms z z + x z against x z + z z: the order does not matter)
      fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
      if (r.limbs != 1 || !same_words(r.buf, cr, (size_t)2 * n)) {
        std::printf("FAIL mul_sum_relin at level 2 differs from fhe_mul_sum_relin_level\n");
        return 1;
      }
    }
    // one term is mul_relin
    for (int rescale = 0; rescale < 2; ++rescale) {
      const fhe::Ciphertext r = ev.mul_sum_relin({&x}, {&z}, rl, rescale != 0);
      const fhe::Ciphertext m = ev.mul_relin(x, z, rl, rescale != 0);
      fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
      if (r.limbs != m.limbs || !same_words(r.buf, m.buf, (size_t)2 * m.limbs * n)) {
        std::printf("FAIL one-term mul_sum_relin (rescale %d) differs from mul_relin\n", rescale);
        return 1;
      }
    }
    // refused at both layers: no terms, 17 terms, rescale at one limb
    const fhe::Ciphertext one = ev.drop_level(x, 1);
    int threw = 0;
    try {
      (void)ev.mul_sum_relin({}, {}, rl, false);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.mul_sum_relin(std::vector<const fhe::Ciphertext*>(17, &x),
                             std::vector<const fhe::Ciphertext*>(17, &x), rl, false);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.mul_sum_relin({&one}, {&one}, rl, true);
    } catch (const fhe::Error&) {
      ++threw;
    }
    fhe::DeviceBuffer c0((size_t)2 * n);
    const uint64_t* p1[1] = {one.data()};
    const uint32_t l1[1] = {1};
    if (threw != 3 || fhe_mul_sum_relin_level(kc.get(), c0.data(), p1, l1, p1, l1, rl.b(), rl.a(), 1, 1,
                                              1, 1, nullptr, nullptr) != FHE_EINVAL) {
      std::printf("FAIL a bad call was not refused\n");
      return 1;
    }
    std::printf("cpp mulsum ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
