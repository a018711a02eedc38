// C++ API for the bootstrap's building blocks (run by tests/test_cpp_bootstrap_ops.py on a GPU
// box): KeyGenerator with a Hamming weight, Evaluator::conj_split and conj_merge at log_n = 10
// compared word for word with residues the Python side computed from oracle/pyoracle.py
// (keygen_secret_sparse, conj_split, conj_merge), and the error codes of the three C entries.
// usage: test_bootstrap_ops FILE seed h level
//   FILE: raw little-endian u64 words over the moduli of Context::standard(10, 4, 2, 2): the
//   expected secret [L + K][N], then ct, cc, re, im, merge(ct, cc), each [2][level][N].
#include <cstdio>
#include <cstdlib>

#include "fhecore.hpp"

using u64 = uint64_t;

int main(int argc, char** argv) {
  if (argc != 5) {
    std::printf("usage: test_bootstrap_ops FILE seed h level\n");
    return 2;
  }
  try {
    const uint32_t log_n = 10, L = 4, K = 2;
    const u64 seed = std::strtoull(argv[2], nullptr, 10);
    const uint32_t h = (uint32_t)std::atoi(argv[3]), level = (uint32_t)std::atoi(argv[4]);
    fhe::Context kc = fhe::Context::standard(log_n, L, K, 2);
    const u64 n = kc.n();
    if (level < 1 || level > L) {
      std::printf("FAIL level out of range\n");
      return 2;
    }
    const size_t sk_words = (size_t)(L + K) * n, ct_words = (size_t)2 * level * n;
    std::vector<u64> sk_want(sk_words);
    std::vector<std::vector<u64>> part(5, std::vector<u64>(ct_words));
    std::FILE* f = std::fopen(argv[1], "rb");
    bool ok = f && std::fread(sk_want.data(), 8, sk_words, f) == sk_words;
    for (auto& p : part) ok = ok && std::fread(p.data(), 8, ct_words, f) == ct_words;
    if (!ok) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    std::fclose(f);

    // the sparse secret
    fhe::KeyGenerator kg(kc, seed, h, nullptr);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (kg.secret().s.download() != sk_want) {
      std::printf("FAIL the sparse secret differs from the reference\n");
      return 1;
    }
    fhe::DeviceBuffer sk(sk_words);
    if (fhe_keygen_secret_sparse(kc.get(), sk.data(), 0, seed, nullptr) != FHE_EINVAL ||
        fhe_keygen_secret_sparse(kc.get(), sk.data(), (uint32_t)n + 1, seed, nullptr) != FHE_EINVAL ||
        fhe_keygen_secret_sparse(kc.get(), nullptr, h, seed, nullptr) != FHE_EINVAL ||
        fhe_keygen_secret_sparse(nullptr, sk.data(), h, seed, nullptr) != FHE_EINVAL) {
      std::printf("FAIL a bad weight or a null pointer was not refused\n");
      return 1;
    }

    // split and merge
    fhe::Evaluator ev(kc);
    fhe::Ciphertext ct(kc, 2, level, true), cc(kc, 2, level, true);
    ct.buf.upload(part[0]);
    cc.buf.upload(part[1]);
    const auto ri = ev.conj_split(ct, cc);
    const fhe::Ciphertext mg = ev.conj_merge(ct, cc);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (ri.first.limbs != level || ri.second.limbs != level || mg.limbs != level ||
        !ri.first.ntt_form || !mg.ntt_form) {
      std::printf("FAIL conj_split / conj_merge returned the wrong shape\n");
      return 1;
    }
    if (ri.first.buf.download() != part[2] || ri.second.buf.download() != part[3]) {
      std::printf("FAIL conj_split differs from the reference\n");
      return 1;
    }
    if (mg.buf.download() != part[4]) {
      std::printf("FAIL conj_merge differs from the reference\n");
      return 1;
    }
    if (ct.buf.download() != part[0] || cc.buf.download() != part[1]) {
      std::printf("FAIL the inputs were written\n");
      return 1;
    }
    // shape mismatches throw; bad levels, null pointers and partial overlaps are FHE_EINVAL
    int threw = 0;
    if (level < L) {
      fhe::Ciphertext other(kc, 2, level + 1, true);
      try {
        (void)ev.conj_split(ct, other);
      } catch (const fhe::Error&) {
        ++threw;
      }
      try {
        (void)ev.conj_merge(other, ct);
      } catch (const fhe::Error&) {
        ++threw;
      }
    } else {
      threw = 2;
    }
    fhe::DeviceBuffer o(2 * ct_words + n);
    u64* re = o.data();
    u64* im = o.data() + ct_words;
    if (threw != 2 ||
        fhe_conj_split_level(kc.get(), re, im, ct.data(), cc.data(), 0, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_split_level(kc.get(), re, im, ct.data(), cc.data(), L + 1, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_split_level(kc.get(), re, nullptr, ct.data(), cc.data(), level, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_split_level(kc.get(), re, re + n, ct.data(), cc.data(), level, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_split_level(kc.get(), ct.data() + n, im, ct.data(), cc.data(), level, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_merge_level(kc.get(), re, ct.data(), cc.data(), 0, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_merge_level(kc.get(), re, ct.data(), cc.data(), L + 1, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_merge_level(kc.get(), nullptr, ct.data(), cc.data(), level, 1, nullptr) != FHE_EINVAL ||
        fhe_conj_merge_level(kc.get(), cc.data() + n, ct.data(), cc.data(), level, 1, nullptr) != FHE_EINVAL) {
      std::printf("FAIL a bad level, a null pointer or an overlap was not refused\n");
      return 1;
    }
    std::printf("cpp bootstrap ops ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
