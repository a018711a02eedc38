// C++ API for batched encryption at any level (run by tests/test_cpp_programs.py on a GPU box):
// Evaluator::encrypt / encrypt_sk with a level and a batch and Evaluator::encrypt_slots compared
// word for word with the C entry points (fhe_encrypt_level, fhe_encrypt_sk_level,
// fhe_encrypt_slots), one top-level ciphertext compared with Evaluator::encrypt, the slots form
// with encode then encrypt, and the refusals at both layers.
#include <cstdio>
#include <cstring>
#include <random>

#include "fhecore.hpp"

using u64 = uint64_t;

static bool same_words(const u64* dev, const std::vector<u64>& want, size_t off, size_t words) {
  std::vector<u64> x(words);
  if (hipMemcpy(x.data(), dev, words * 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
  return std::memcmp(x.data(), want.data() + off, words * 8) == 0;
}

int main() {
  try {
    const uint32_t log_n = 10, L = 4, batch = 3, index0 = 5;
    const u64 seed = 0x1234567887654321ull;
    fhe::Context kc = fhe::Context::standard(log_n, L, 2, 2);
    const u64 n = kc.n();
    fhe::KeyGenerator kg(kc, 42);
    const fhe::PublicKey pk = kg.public_key(43);
    fhe::Evaluator ev(kc);
    std::vector<u64> q(L + 2);
    fhe::check(fhe_ctx_moduli(kc.get(), q.data(), nullptr), "moduli");
    std::mt19937_64 rng(13);
    std::vector<u64> h((size_t)L * n);
    for (uint32_t l = 0; l < L; ++l)
      for (u64 i = 0; i < n; ++i) h[(size_t)l * n + i] = rng() % q[l];
    fhe::Ciphertext pt(kc, 1, L, true);
    pt.buf.upload(h);
    auto sync = [] { fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync"); };

    for (uint32_t level : {2u, L}) {
      const size_t words = (size_t)2 * level * n;
      fhe::DeviceBuffer c(words * batch);
      for (int secret = 0; secret < 2; ++secret) {
        const std::vector<fhe::Ciphertext> got =
            secret ? ev.encrypt_sk(&pt, kg.secret(), level, batch, seed, index0)
                   : ev.encrypt(&pt, pk, level, batch, seed, index0);
        fhe::check(secret ? fhe_encrypt_sk_level(kc.get(), c.data(), pt.data(), L, 1,
                                                 kg.secret().s.data(), level, batch, seed, index0,
                                                 nullptr, nullptr)
                          : fhe_encrypt_level(kc.get(), c.data(), pt.data(), L, 1, pk.pk.data(),
                                              level, batch, seed, index0, nullptr, nullptr),
                   "fhe_encrypt_level");
        sync();
        const std::vector<u64> want = c.download();
        if (got.size() != batch) return std::printf("FAIL batch size\n"), 1;
        for (uint32_t i = 0; i < batch; ++i)
          if (got[i].components != 2 || got[i].limbs != level || !got[i].ntt_form ||
              !same_words(got[i].data(), want, i * words, words)) {
            std::printf("FAIL encrypt (secret %d, level %u) differs from the C entry point\n", secret,
                        level);
            return 1;
          }
      }
    }
    // one ciphertext, index0 = 0, level L: Evaluator::encrypt; and a null plaintext is zero
    {
      const fhe::Ciphertext old = ev.encrypt(pt, pk, seed);
      const std::vector<fhe::Ciphertext> one = ev.encrypt(&pt, pk, L, 1, seed);
      sync();
      if (!same_words(one[0].data(), old.buf.download(), 0, (size_t)2 * L * n)) {
        std::printf("FAIL the batched encrypt's element 0 differs from Evaluator::encrypt\n");
        return 1;
      }
      fhe::Ciphertext zero(kc, 1, L, true);
      zero.buf.upload(std::vector<u64>((size_t)L * n, 0));
      const std::vector<fhe::Ciphertext> a = ev.encrypt_sk(nullptr, kg.secret(), L, 2, seed);
      const std::vector<fhe::Ciphertext> b = ev.encrypt_sk(&zero, kg.secret(), L, 2, seed);
      sync();
      if (!same_words(a[1].data(), b[1].buf.download(), 0, (size_t)2 * L * n)) {
        std::printf("FAIL a null plaintext is not an encryption of zero\n");
        return 1;
      }
    }
    // the slots form: encode then encrypt, full packing and 8 slots, both keys
    for (uint32_t log_slots : {log_n - 1, 3u}) {
      const size_t ns2 = (size_t)2 << log_slots;
      std::vector<u64> zs(ns2 * batch);
      std::uniform_real_distribution<double> uni(-1.0, 1.0);
      for (auto& w : zs) {
        const double v = uni(rng);
        std::memcpy(&w, &v, 8);
      }
      fhe::DeviceBuffer slots(ns2 * batch);
      slots.upload(zs);
      const uint32_t level = 3;
      const size_t words = (size_t)2 * level * n;
      for (int secret = 0; secret < 2; ++secret) {
        const std::vector<fhe::Ciphertext> got =
            secret ? ev.encrypt_slots(slots, 0x1p50, log_slots, kg.secret(), level, batch, seed, index0)
                   : ev.encrypt_slots(slots, 0x1p50, log_slots, pk, level, batch, seed, index0);
        fhe::DeviceBuffer c(words * batch);
        fhe::check(fhe_encrypt_slots(kc.get(), c.data(), reinterpret_cast<const double*>(slots.data()),
                                     0x1p50, log_slots, secret ? kg.secret().s.data() : pk.pk.data(),
                                     secret, level, batch, seed, index0, nullptr, nullptr),
                   "fhe_encrypt_slots");
        sync();
        const std::vector<u64> want = c.download();
        for (uint32_t i = 0; i < batch; ++i) {
          fhe::DeviceBuffer zi(ns2);
          zi.upload(std::vector<u64>(zs.begin() + i * ns2, zs.begin() + (i + 1) * ns2));
          const fhe::Ciphertext p = ev.encode(zi, 0x1p50, log_slots, level, false);
          const std::vector<fhe::Ciphertext> two =
              secret ? ev.encrypt_sk(&p, kg.secret(), level, 1, seed, index0 + i)
                     : ev.encrypt(&p, pk, level, 1, seed, index0 + i);
          sync();
          if (!same_words(got[i].data(), want, i * words, words) ||
              !same_words(two[0].data(), want, i * words, words)) {
            std::printf("FAIL encrypt_slots (secret %d, log_slots %u) element %u\n", secret, log_slots, i);
            return 1;
          }
        }
      }
    }
    // refused at both layers
    int threw = 0;
    try {
      (void)ev.encrypt(&pt, pk, 0, 1, seed);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.encrypt_sk(&pt, kg.secret(), L + 1, 1, seed);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      fhe::DeviceBuffer zb(n);
      zb.upload(std::vector<u64>(n, 0));
      const fhe::Ciphertext low = ev.encode(zb, 0x1p50, 2);
      (void)ev.encrypt(&low, pk, 3, 1, seed);  // a plaintext below the level
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.encrypt_slots(fhe::DeviceBuffer(16), 0x1p50, 3, pk, L, 2, seed);  // slots for one
    } catch (const fhe::Error&) {
      ++threw;
    }
    fhe::DeviceBuffer c0((size_t)2 * L * n);
    if (threw != 4 ||
        fhe_encrypt_level(kc.get(), c0.data(), pt.data(), L, 1, pk.pk.data(), L, 2, seed, 0xffffffffu,
                          nullptr, nullptr) != FHE_EINVAL ||
        fhe_encrypt_level(kc.get(), c0.data(), pt.data(), L, 2, pk.pk.data(), L, 1, seed, 0, nullptr,
                          nullptr) != FHE_EINVAL) {
      std::printf("FAIL a bad call was not refused (%d)\n", threw);
      return 1;
    }
    std::printf("cpp encrypt ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
