// C++ API at levels below the top (run by tests/test_cpp_programs.py on a GPU box): two
// Evaluator::mul_relin(rescale) in a row, L = 3 -> 2 -> 1 limbs, and a rotation at 2 limbs, compared
// word for word with the C entry points (fhe_mul_relin, fhe_mul_relin_level, fhe_rotate_level).
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
    const uint32_t log_n = 10, L = 3;
    fhe::Context kc = fhe::Context::standard(log_n, L, 2, 3);
    const u64 n = kc.n();
    fhe::KeyGenerator kg(kc, 42);
    const fhe::PublicKey pk = kg.public_key(43);
    const fhe::SwitchKey rl = kg.relin_key(46);
    fhe::Evaluator ev(kc);
    std::vector<u64> q(L + 2);
    fhe::check(fhe_ctx_moduli(kc.get(), q.data(), nullptr), "moduli");
    std::mt19937_64 rng(9);
    std::vector<u64> hp(L * n);
    for (uint32_t l = 0; l < L; ++l)
      for (u64 i = 0; i < n; ++i) hp[l * n + i] = rng() % q[l];
    fhe::Ciphertext pt(kc, 1, L, true);
    pt.buf.upload(hp);
    const fhe::Ciphertext x = ev.encrypt(pt, pk, 44);

    // through the Evaluator: the level is the ciphertext's limb count
    const fhe::Ciphertext y = ev.mul_relin(x, x, rl, true);
    const fhe::Ciphertext z = ev.mul_relin(y, y, rl, true);
    if (y.limbs != L - 1 || z.limbs != L - 2) {
      std::printf("FAIL mul_relin shapes %u %u\n", y.limbs, z.limbs);
      return 1;
    }
    // the same through the C entry points (internal workspace)
    fhe::DeviceBuffer cy((size_t)2 * (L - 1) * n), cz((size_t)2 * (L - 2) * n);
    fhe::check(fhe_mul_relin(kc.get(), cy.data(), x.data(), x.data(), rl.b(), rl.a(), 1, 1, nullptr,
                             nullptr),
               "fhe_mul_relin");
    fhe::check(fhe_mul_relin_level(kc.get(), cz.data(), cy.data(), cy.data(), rl.b(), rl.a(), L - 1, 1,
                                   1, nullptr, nullptr),
               "fhe_mul_relin_level");
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (!same_words(y.buf, cy, (size_t)2 * (L - 1) * n)) {
      std::printf("FAIL first mul_relin differs from fhe_mul_relin\n");
      return 1;
    }
    if (!same_words(z.buf, cz, (size_t)2 * (L - 2) * n)) {
      std::printf("FAIL second mul_relin differs from fhe_mul_relin_level\n");
      return 1;
    }
    // a rotation at 2 limbs with the top-level rotation key
    const uint32_t k = ev.galois_elt(1);
    const fhe::SwitchKey rk = kg.rotation_key(k, 45);
    const fhe::Ciphertext r = ev.rotate(y, k, rk);
    fhe::DeviceBuffer cr((size_t)2 * (L - 1) * n);
    fhe::check(fhe_rotate_level(kc.get(), cr.data(), cy.data(), k, rk.b(), rk.a(), L - 1, 1, nullptr,
                                nullptr),
               "fhe_rotate_level");
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (r.limbs != L - 1 || !same_words(r.buf, cr, (size_t)2 * (L - 1) * n)) {
      std::printf("FAIL rotate at 2 limbs differs from fhe_rotate_level\n");
      return 1;
    }
    // rescale with one limb left is refused, at both layers
    bool threw = false;
    try {
      (void)ev.mul_relin(z, z, rl, true);
    } catch (const fhe::Error&) {
      threw = true;
    }
    fhe::DeviceBuffer c0((size_t)2 * n);
    if (!threw || fhe_mul_relin_level(kc.get(), c0.data(), cz.data(), cz.data(), rl.b(), rl.a(), 1, 1, 1,
                                      nullptr, nullptr) != FHE_EINVAL) {
      std::printf("FAIL rescale at one limb was not refused\n");
      return 1;
    }
    std::printf("cpp levels ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
