// C++ API for decrypting straight to slots (run by tests/test_cpp_decrypt_slots.py on a GPU box):
// Evaluator::encrypt_slots -> Evaluator::decrypt_slots at log_n = 10, full packing and 8 slots,
// compared word for word with what the Python side computed from tests/encrypt_ref.py and the
// decoders' references, and with Evaluator::decode(Evaluator::decrypt(ct)) inside the program.
// usage: test_decrypt_slots FILE
//   FILE: raw little-endian 64-bit words: the slots [N/2][2] doubles and [8][2] doubles, then the
//   expected results in the same shapes, for Context::standard(10, 4, 2, 2), the secret of
//   KeyGenerator seed 42, secret-key encryption at level 3 with seed 0x1234567887654321 and
//   index0 5, delta = 2^50.
#include <cstdio>
#include <cstdlib>

#include "fhecore.hpp"

using u64 = uint64_t;

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: test_decrypt_slots FILE\n");
    return 2;
  }
  try {
    const uint32_t log_n = 10, L = 4, K = 2, level = 3, index0 = 5, sparse = 3;
    const u64 seed = 0x1234567887654321ull;
    const double delta = 0x1p50;
    fhe::Context kc = fhe::Context::standard(log_n, L, K, 2);
    const u64 n = kc.n();
    const size_t ns2 = (size_t)2 << sparse;
    std::vector<u64> zf(n), zs(ns2), want_f(n), want_s(ns2);
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(zf.data(), 8, n, f) != n || std::fread(zs.data(), 8, ns2, f) != ns2 ||
        std::fread(want_f.data(), 8, n, f) != n || std::fread(want_s.data(), 8, ns2, f) != ns2) {
      std::printf("FAIL cannot read %s\n", argv[1]);
      return 2;
    }
    std::fclose(f);
    fhe::KeyGenerator kg(kc, 42);
    fhe::Evaluator ev(kc);
    auto sync = [] { fhe::check(hipDeviceSynchronize() == hipSuccess ? FHE_OK : FHE_EDEVICE, "sync"); };

    fhe::DeviceBuffer z(n), zz(ns2);
    z.upload(zf);
    zz.upload(zs);
    const fhe::Ciphertext ct =
        std::move(ev.encrypt_slots(z, delta, log_n - 1, kg.secret(), level, 1, seed, index0)[0]);
    const fhe::Ciphertext cs =
        std::move(ev.encrypt_slots(zz, delta, sparse, kg.secret(), level, 1, seed, index0)[0]);
    sync();
    const std::vector<u64> ct_before = ct.buf.download(), sk_before = kg.secret().s.download();

    const fhe::DeviceBuffer full = ev.decrypt_slots(ct, kg.secret(), delta);
    const fhe::DeviceBuffer full2 = ev.decrypt_slots(ct, kg.secret(), delta, log_n - 1);
    const fhe::DeviceBuffer few = ev.decrypt_slots(cs, kg.secret(), delta, sparse);
    sync();
    if (full.size() != n || few.size() != ns2) {
      std::printf("FAIL decrypt_slots returned the wrong size\n");
      return 1;
    }
    if (full.download() != want_f || full2.download() != want_f) {
      std::printf("FAIL decrypt_slots (full packing) differs from the reference\n");
      return 1;
    }
    if (few.download() != want_s) {
      std::printf("FAIL decrypt_slots (8 slots) differs from the reference\n");
      return 1;
    }
    // the composed calls
    const fhe::DeviceBuffer cf = ev.decode(ev.decrypt(ct, kg.secret()), delta, level);
    const fhe::DeviceBuffer cfew = ev.decode(ev.decrypt(cs, kg.secret()), delta, sparse, level);
    sync();
    if (cf.download() != want_f || cfew.download() != want_s) {
      std::printf("FAIL decode(decrypt(ct)) differs from decrypt_slots\n");
      return 1;
    }
    if (ct.buf.download() != ct_before || kg.secret().s.download() != sk_before) {
      std::printf("FAIL decrypt_slots wrote an input\n");
      return 1;
    }
    // refused at both layers
    int threw = 0;
    try {
      (void)ev.decrypt_slots(ct, kg.secret(), delta, log_n);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.decrypt_slots(ct, kg.secret(), -1.0);
    } catch (const fhe::Error&) {
      ++threw;
    }
    try {
      (void)ev.decrypt_slots(ev.decrypt(ct, kg.secret()), kg.secret(), delta);  // one component
    } catch (const fhe::Error&) {
      ++threw;
    }
    fhe::DeviceBuffer o(n), ws(3 * n);
    double* op = reinterpret_cast<double*>(o.data());
    if (threw != 3 ||
        fhe_decrypt_slots(kc.get(), op, ct.data(), kg.secret().s.data(), delta, log_n - 1, L + 1, 1,
                          ws.data(), nullptr) != FHE_EINVAL ||
        fhe_decrypt_slots(kc.get(), op, ct.data(), kg.secret().s.data(), delta, log_n - 1, 0, 1,
                          ws.data(), nullptr) != FHE_EINVAL ||
        fhe_decrypt_slots(kc.get(), reinterpret_cast<double*>(ws.data()), ct.data(),
                          kg.secret().s.data(), delta, log_n - 1, level, 1, ws.data(),
                          nullptr) != FHE_EINVAL ||
        fhe_decrypt_slots(kc.get(), op, ct.data(), kg.secret().s.data(), delta, log_n - 1, level, 0,
                          ws.data(), nullptr) != FHE_OK) {
      std::printf("FAIL bad arguments or an overlap were not refused (%d)\n", threw);
      return 1;
    }
    std::printf("cpp decrypt_slots ok\n");
    return 0;
  } catch (const std::exception& e) {
    std::printf("FAIL exception: %s\n", e.what());
    return 1;
  }
}
