// C++ API for sparse packing (run by tests/test_cpp_sparse_pack.py on a GPU box): the
// Evaluator::encode and decode overloads with log_slots at log_n = 10, compared word for word with
// what the Python side computed from tests/sparse_pack_ref.py.
// usage: test_sparse_pack FILE log_slots level special
//   FILE: raw little-endian 64-bit words: the slots [n_s][2] doubles, the expected plaintext
//   [level (+ K)][N] and the expected decoded slots [n_s][2] doubles, over the moduli of
//   Context::standard(10, 4, 2, 2) at delta = 2^50.
#include <cstdio>
#include <cstdlib>

#include "fhecore.hpp"

using u64 = uint64_t;

int main(int argc, char** argv) {
  if (argc != 5) {
    std::printf("usage: test_sparse_pack FILE log_slots level special\n");
    return 2;
  }
  try {
    const uint32_t log_n = 10, L = 4, K = 2;
    const double delta = 1125899906842624.0;  // 2^50
    const uint32_t ls = (uint32_t)std::atoi(argv[2]);
    const uint32_t level = (uint32_t)std::atoi(argv[3]);
    const bool special = std::atoi(argv[4]) != 0;
    fhe::Context kc = fhe::Context::standard(log_n, L, K, 2);
    const u64 n = kc.n();
    if (level < 1 || level > L || ls > log_n - 1) {
      std::printf("FAIL level or log_slots out of range\n");
      return 2;
    }
    const size_t zw = (size_t)2 << ls;  // words of the slot vector
    const uint32_t rows = level + (special ? K : 0);
    const size_t pt_words = (size_t)rows * n;
    std::vector<u64> hz(zw), want(pt_words), want_back(zw);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(hz.data(), 8, zw, f) != zw ||
        std::fread(want.data(), 8, pt_words, f) != pt_words ||
        std::fread(want_back.data(), 8, zw, f) != zw) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    std::fclose(f);
    fhe::Evaluator ev(kc);
    fhe::DeviceBuffer z(zw);
    z.upload(hz);
    const fhe::Ciphertext pt = ev.encode(z, delta, ls, level, special);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (pt.limbs != rows || pt.components != 1 || !pt.ntt_form || pt.buf.size() != pt_words) {
      std::printf("FAIL encode returned the wrong shape\n");
      return 1;
    }
    const std::vector<u64> got = pt.buf.download();
    for (size_t i = 0; i < pt_words; ++i)
      if (got[i] != want[i]) {
        std::printf("FAIL sparse encode differs from the reference at word %zu\n", i);
        return 1;
      }
    if (z.download() != hz) {
      std::printf("FAIL encode wrote its input\n");
      return 1;
    }
    const fhe::DeviceBuffer back = ev.decode(pt, delta, ls, level);
    fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync");
    if (back.size() != zw || back.download() != want_back) {
      std::printf("FAIL sparse decode differs from the reference\n");
      return 1;
    }
    // a log_slots above log_n - 1, a slot buffer of another size and a bad scale are refused
    int threw = 0;
    try {
      (void)ev.encode(z, delta, log_n, level, special);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.decode(pt, delta, log_n, level);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.encode(z, delta, ls == 0 ? 1 : ls - 1, level, special);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.encode(z, -1.0, ls, level, special);
    } catch (const fhe::Error&) {
      ++threw;
    }
    fhe::DeviceBuffer o(pt_words), ws(3 * n);
    const double* zp = reinterpret_cast<const double*>(z.data());
    if (threw != 4 ||
        fhe_encode_sparse(kc.get(), o.data(), zp, delta, log_n, level, 0, 1, ws.data(), nullptr) !=
            FHE_EINVAL ||
        fhe_encode_sparse(kc.get(), z.data(), zp, delta, ls, level, 0, 1, ws.data(), nullptr) !=
            FHE_EINVAL ||
        fhe_decode_sparse(kc.get(), reinterpret_cast<double*>(o.data()), pt.data(), delta, log_n,
                          rows, level, 1, ws.data(), nullptr) != FHE_EINVAL) {
      std::printf("FAIL bad arguments or an overlap were not refused\n");
      return 1;
    }
    std::printf("cpp sparse pack ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
