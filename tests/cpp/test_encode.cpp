// C++ API for the device encoder / decoder (run by tests/test_cpp_encode.py on a GPU box):
// Evaluator::encode and decode at log_n = 10 compared word for word with what the Python side
// computed from tests/encode_ref.py.
// usage: test_encode FILE level special
//   FILE: raw little-endian 64-bit words: the slots [N/2][2] doubles, the expected plaintext
//   [level (+ K)][N] and the expected decoded slots [N/2][2] doubles, over the moduli of
//   Context::standard(10, 4, 2, 2) at delta = 2^50.
#include <cstdio>
#include <cstdlib>

#include "fhecore.hpp"

using u64 = uint64_t;

int main(int argc, char** argv) {
  if (argc != 4) {
    std::printf("usage: test_encode FILE level special\n");
    return 2;
  }
  try {
    const uint32_t log_n = 10, L = 4, K = 2;
    const double delta = 1125899906842624.0;  // 2^50
    const uint32_t level = (uint32_t)std::atoi(argv[2]);
    const bool special = std::atoi(argv[3]) != 0;
    fhe::Context kc = fhe::Context::standard(log_n, L, K, 2);
    const u64 n = kc.n();
    if (level < 1 || level > L) {
      std::printf("FAIL level out of range\n");
      return 2;
    }
    const uint32_t rows = level + (special ? K : 0);
    const size_t pt_words = (size_t)rows * n;
    std::vector<u64> hz(n), want(pt_words), want_back(n);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(hz.data(), 8, n, f) != n ||
        std::fread(want.data(), 8, pt_words, f) != pt_words ||
        std::fread(want_back.data(), 8, n, f) != n) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    std::fclose(f);
    fhe::Evaluator ev(kc);
    fhe::DeviceBuffer z(n);
    z.upload(hz);
    const fhe::Ciphertext pt = ev.encode(z, delta, level, special);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (pt.limbs != rows || pt.components != 1 || !pt.ntt_form || pt.buf.size() != pt_words) {
      std::printf("FAIL encode returned the wrong shape\n");
      return 1;
    }
    const std::vector<u64> got = pt.buf.download();
    for (size_t i = 0; i < pt_words; ++i)
      if (got[i] != want[i]) {
        std::printf("FAIL encode differs from the reference at word %zu\n", i);
        return 1;
      }
    if (z.download() != hz) {
      std::printf("FAIL encode wrote its input\n");
      return 1;
    }
    const fhe::DeviceBuffer back = ev.decode(pt, delta, level);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (back.download() != want_back) {
      std::printf("FAIL decode differs from the reference\n");
      return 1;
    }
    // bad levels and a bad scale are refused, at both layers
    int threw = 0;
    for (uint32_t bad : {0u, L + 1}) {
      try {
        (void)ev.encode(z, delta, bad, special);
      } catch (const fhe::Error&) {
        ++threw;
      }
      try {
        (void)ev.decode(pt, delta, bad);
      } catch (const fhe::Error&) {
        ++threw;
      }
    }
    try {
      (void)ev.encode(z, -1.0, level, special);
    } catch (const fhe::Error&) {
      ++threw;
    }
    fhe::DeviceBuffer o(pt_words), ws(3 * n);
    const double* zp = reinterpret_cast<const double*>(z.data());
    if (threw != 5 ||
        fhe_encode(kc.get(), o.data(), zp, delta, L + 1, 0, 1, ws.data(), nullptr) != FHE_EINVAL ||
        fhe_encode(kc.get(), z.data(), zp, delta, level, 0, 1, ws.data(), nullptr) != FHE_EINVAL ||
        fhe_decode(kc.get(), reinterpret_cast<double*>(o.data()), pt.data(), delta, 1, 2, 1,
                   ws.data(), nullptr) != FHE_EINVAL) {
      std::printf("FAIL bad arguments or an overlap were not refused\n");
      return 1;
    }
    std::printf("cpp encode ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
