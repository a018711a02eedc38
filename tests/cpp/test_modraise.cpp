// C++ API for ModRaise (run by tests/test_cpp_modraise.py on a GPU box): Evaluator::mod_raise at
// log_n = 10 compared word for word with residues the Python side computed from
// oracle/pyoracle.py (mod_raise).
// usage: test_modraise FILE in_level out_level
//   FILE: raw little-endian u64 words, the input [2][in_level][N] then the expected output
//   [2][out_level][N], over the moduli of Context::standard(10, 4, 2, 2).
#include <cstdio>
#include <cstdlib>

#include "fhecore.hpp"

using u64 = uint64_t;

int main(int argc, char** argv) {
  if (argc != 4) {
    std::printf("usage: test_modraise FILE in_level out_level\n");
    return 2;
  }
  try {
    const uint32_t log_n = 10, L = 4;
    const uint32_t in_level = (uint32_t)std::atoi(argv[2]), out_level = (uint32_t)std::atoi(argv[3]);
    fhe::Context kc = fhe::Context::standard(log_n, L, 2, 2);
    const u64 n = kc.n();
    if (in_level < 1 || in_level > L || out_level < 1 || out_level > L) {
      std::printf("FAIL levels out of range\n");
      return 2;
    }
    const size_t in_words = (size_t)2 * in_level * n, out_words = (size_t)2 * out_level * n;
    std::vector<u64> hin(in_words), want(out_words);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(hin.data(), 8, in_words, f) != in_words ||
        std::fread(want.data(), 8, out_words, f) != out_words) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    std::fclose(f);
    fhe::Evaluator ev(kc);
    fhe::Ciphertext ct(kc, 2, in_level, true);
    ct.buf.upload(hin);
    const fhe::Ciphertext up = ev.mod_raise(ct, out_level);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    const std::vector<u64> got = up.buf.download();
    if (up.limbs != out_level || up.components != 2 || !up.ntt_form || got.size() != out_words) {
      std::printf("FAIL mod_raise returned the wrong shape\n");
      return 1;
    }
    for (size_t i = 0; i < out_words; ++i)
      if (got[i] != want[i]) {
        std::printf("FAIL mod_raise differs from the reference at word %zu\n", i);
        return 1;
      }
    // the input is untouched
    if (ct.buf.download() != hin) {
      std::printf("FAIL mod_raise wrote its input\n");
      return 1;
    }
    // bad levels are refused, at both layers
    int threw = 0;
    for (uint32_t bad : {0u, L + 1}) {
      try {
        (void)ev.mod_raise(ct, bad);
      } catch (const fhe::Error&) {
        ++threw;
      }
    }
    fhe::DeviceBuffer o(out_words), ws(2 * n);
    if (threw != 2 ||
        fhe_mod_raise(kc.get(), o.data(), ct.data(), in_level, L + 1, 1, ws.data(), nullptr) !=
            FHE_EINVAL ||
        fhe_mod_raise(kc.get(), o.data(), ct.data(), 0, out_level, 1, ws.data(), nullptr) !=
            FHE_EINVAL ||
        fhe_mod_raise(kc.get(), ct.data(), ct.data(), in_level, out_level, 1, ws.data(), nullptr) !=
            FHE_EINVAL) {
      std::printf("FAIL bad levels or an overlap were not refused\n");
      return 1;
    }
    std::printf("cpp modraise ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
