// C++ API for the hoisted rotations and the rotation sum below the top level (run by
// tests/test_cpp_programs.py on a GPU box): a ciphertext brought from L = 4 to 2 limbs by two
// Evaluator::mul_relin(rescale), then Evaluator::rotate_hoisted and Evaluator::rotate_sum at those
// 2 limbs with the top-level keys and plaintexts, compared word for word with the C entry points
// (fhe_rotate_hoisted_level, fhe_rotate_sum_hoisted_level).
#include <cstdio>
#include <random>

#include "fhecore.hpp"

using u64 = uint64_t;

static bool same_words(const u64* a, const u64* b, size_t words) {
  std::vector<u64> x(words), y(words);
  if (hipMemcpy(x.data(), a, words * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(y.data(), b, words * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return false;
  for (size_t i = 0; i < words; ++i)
    if (x[i] != y[i]) return false;
  return true;
}

int main() {
  try {
    const uint32_t log_n = 10, L = 4, K = 2, level = L - 2;
    fhe::Context kc = fhe::Context::standard(log_n, L, K, 2);
    const u64 n = kc.n();
    fhe::KeyGenerator kg(kc, 52);
    const fhe::PublicKey pk = kg.public_key(53);
    const fhe::SwitchKey rl = kg.relin_key(54);
    fhe::Evaluator ev(kc);
    std::vector<u64> q(L + K);
    fhe::check(fhe_ctx_moduli(kc.get(), q.data(), nullptr), "moduli");
    std::mt19937_64 rng(19);
    std::vector<u64> hp(L * n);
    for (uint32_t l = 0; l < L; ++l)
      for (u64 i = 0; i < n; ++i) hp[l * n + i] = rng() % q[l];
    fhe::Ciphertext pt(kc, 1, L, true);
    pt.buf.upload(hp);
    const fhe::Ciphertext x = ev.encrypt(pt, pk, 55);
    const fhe::Ciphertext y = ev.mul_relin(x, x, rl, true);
    const fhe::Ciphertext z = ev.mul_relin(y, y, rl, true);
    if (z.limbs != level) {
      std::printf("FAIL mul_relin chain left %u limbs\n", z.limbs);
      return 1;
    }
    const size_t words = (size_t)2 * level * n;

    // hoisted rotations at 2 limbs with the top-level rotation keys
    const uint32_t k1 = ev.galois_elt(1), k2 = ev.galois_elt(-3);
    const fhe::SwitchKey rk1 = kg.rotation_key(k1, 56), rk2 = kg.rotation_key(k2, 57);
    const std::vector<uint32_t> elts{k1, k2};
    const std::vector<fhe::Ciphertext> rot = ev.rotate_hoisted(z, elts, {&rk1, &rk2});
    fhe::DeviceBuffer ch(2 * words);
    const u64* kb[2] = {rk1.b(), rk2.b()};
    const u64* ka[2] = {rk1.a(), rk2.a()};
    fhe::check(fhe_rotate_hoisted_level(kc.get(), ch.data(), z.data(), elts.data(), kb, ka, level, 2,
                                        1, nullptr, nullptr),
               "fhe_rotate_hoisted_level");
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (rot.size() != 2 || rot[0].limbs != level || rot[1].limbs != level ||
        !same_words(rot[0].data(), ch.data(), words) ||
        !same_words(rot[1].data(), ch.data() + words, words)) {
      std::printf("FAIL rotate_hoisted at 2 limbs differs from fhe_rotate_hoisted_level\n");
      return 1;
    }

    // the rotation sum at 2 limbs: plaintexts [L + K][N] over Q u P, as at the top level
    fhe::DeviceBuffer p0((size_t)(L + K) * n), p1((size_t)(L + K) * n);
    for (fhe::DeviceBuffer* p : {&p0, &p1}) {
      std::vector<u64> h((L + K) * n);
      for (uint32_t l = 0; l < L + K; ++l)
        for (u64 i = 0; i < n; ++i) h[l * n + i] = rng() % q[l];
      p->upload(h);
    }
    const std::vector<uint32_t> terms{1, k1};
    const fhe::Ciphertext sum = ev.rotate_sum(z, terms, {nullptr, &rk1}, {&p0, &p1});
    fhe::DeviceBuffer cs(words);
    const u64* sb[2] = {nullptr, rk1.b()};
    const u64* sa[2] = {nullptr, rk1.a()};
    const u64* sp[2] = {p0.data(), p1.data()};
    fhe::check(fhe_rotate_sum_hoisted_level(kc.get(), cs.data(), z.data(), terms.data(), sb, sa, sp,
                                            level, 2, 1, nullptr, nullptr),
               "fhe_rotate_sum_hoisted_level");
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (sum.limbs != level || !same_words(sum.data(), cs.data(), words)) {
      std::printf("FAIL rotate_sum at 2 limbs differs from fhe_rotate_sum_hoisted_level\n");
      return 1;
    }
    // a level outside [1, L] is refused by the C entry point
    if (fhe_rotate_sum_hoisted_level(kc.get(), cs.data(), z.data(), terms.data(), sb, sa, sp, L + 1,
                                     2, 1, nullptr, nullptr) != FHE_EINVAL) {
      std::printf("FAIL level L + 1 was not refused\n");
      return 1;
    }
    std::printf("cpp level hoist ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
