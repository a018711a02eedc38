"""Context / Ciphertext / Evaluator: the host-side API over libfhecore.

SURVEY.md §8b asks for a Context/Ciphertext/Evaluator layer above the C ABI (the reference has
no such layer: it passes ``MOD`` per call, /root/reference/arithmetic.py:3-13).  Device memory,
streams and multi-GPU collectives are PyTorch-ROCm plumbing; every arithmetic operation is a
libfhecore call into hand-written gfx950 kernels.  Tensors are int64 views of the uint64
residues, layout [..., limb, N], on a HIP device.
"""
from __future__ import annotations

import ctypes
import secrets
import threading
from fractions import Fraction
from functools import lru_cache

import numpy as np

from . import _capi
from ._capi import check, load

try:  # torch is the device-memory / stream provider
    import torch
except ImportError:  # pragma: no cover - the image always has torch
    torch = None


# ----------------------------------------------------------------------------- parameters

@lru_cache(maxsize=None)
def _gen_moduli_cached(log_n: int, count: int, bits: int, skip: int) -> tuple:
    out = (ctypes.c_uint64 * count)()
    check(load().fhe_gen_moduli(log_n, count, bits, skip, out), "fhe_gen_moduli")
    return tuple(int(v) for v in out)


def gen_moduli(log_n: int, count: int, bits: int = 60, skip: int = 0) -> list:
    """SURVEY.md §8a' modulus chain: the largest primes < 2^bits, q = 1 mod 2N, descending."""
    return list(_gen_moduli_cached(log_n, count, bits, skip))


def default_params(log_n: int, L: int, K: int = 0):
    """(Q-moduli, P-moduli): L + K consecutive primes of the §8a' chain."""
    m = gen_moduli(log_n, L + K)
    return m[:L], m[L:]


def encode_roots(log_n: int) -> np.ndarray:
    """The special FFT's root table of a context at ring degree 2^log_n (fhe_encode_roots; no
    device needed): float64 [2N, 2], row k = (cos, sin)(pi k / N), the values the context uploads
    for fhe_encode / fhe_decode."""
    out = np.empty((2 << log_n, 2), dtype=np.float64)
    check(load().fhe_encode_roots(log_n, out.ctypes.data_as(ctypes.c_void_p)), "fhe_encode_roots")
    return out


# ----------------------------------------------------------------------------- device helpers

def _nonce(seed):
    """The Philox seed of one keygen/encryption call: a fresh CSPRNG draw unless given."""
    return secrets.randbits(64) if seed is None else int(seed)


def _require_device():
    if torch is None or not torch.cuda.is_available():
        raise _capi.FheError("fhecore needs a HIP device (torch.cuda.is_available() is False); "
                             "there is no CPU fallback")


def to_device(x, device=None):
    """numpy uint64/int64 (or any integer array with values in [0, 2^64)) -> int64 device tensor."""
    _require_device()
    if isinstance(x, torch.Tensor):
        return x.to(device or "cuda").contiguous()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a.view(np.int64)).to(device or "cuda")


def to_host(t) -> np.ndarray:
    """int64 device tensor -> numpy uint64 array."""
    return t.detach().to("cpu").contiguous().numpy().view(np.uint64)


def _ptr(t) -> int:
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _check_tensor(t, what, shape_tail=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{what}: expected a HIP device tensor")
    if t.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{what}: expected int64/uint64 residues, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: tensor must be contiguous")
    if shape_tail is not None and tuple(t.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise ValueError(f"{what}: trailing shape {tuple(t.shape)} != (..., {shape_tail})")


def _check_out(out, ref, shape, what):
    """A caller-supplied output: its raw pointer goes straight to a kernel, so it must be a
    contiguous int64/uint64 HIP tensor of exactly `shape` on the device of `ref` (a CPU tensor or
    one on another GPU would be written through an invalid device address)."""
    _check_tensor(out, what)
    if out.device != ref.device:
        raise ValueError(f"{what}: on {out.device}, the inputs are on {ref.device}")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{what}: shape {tuple(out.shape)} != {tuple(shape)}")
    return out


# ----------------------------------------------------------------------------- context

# Tensors allocated by this module while a Graph is capturing: the captured kernels keep their
# addresses, so the Graph holds a reference to each (else the caching allocator would hand their
# memory to other tensors while replays still write it).
_CAPTURE = threading.local()


def _keep(t):
    keep = getattr(_CAPTURE, "keep", None)
    if keep is not None:
        keep.append(t)
    return t


def _empty(*args, **kw):
    return _keep(torch.empty(*args, **kw))


def _empty_like(*args, **kw):
    return _keep(torch.empty_like(*args, **kw))


class Context:
    """RNS-CKKS-style parameter context on one HIP device (wraps ``fhe_ctx``).

    moduli: Q-primes (L of them); special: P-primes (K, for key-switching); dnum gadget digits.
    Defaults follow SURVEY.md §8a' (``default_params``).
    """

    def __init__(self, log_n: int, moduli=None, special=None, dnum: int = 1, L: int = None,
                 K: int = 0, device: int = None):
        _require_device()
        lib = load()
        if moduli is None:
            if L is None:
                raise ValueError("give moduli or L")
            moduli, dflt_special = default_params(log_n, L, K)
            if special is None:
                special = dflt_special
        special = list(special or [])
        moduli = [int(q) for q in moduli]
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.log_n = int(log_n)
        self.n = 1 << self.log_n
        self.L, self.K = len(moduli), len(special)
        self.dnum = int(dnum) if self.K else 0
        self.alpha = -(-self.L // self.dnum) if self.K else 0
        self._ptr = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.fhe_ctx_create(ctypes.byref(self._ptr), self.log_n, _capi.u64_array(moduli),
                                     self.L, _capi.u64_array(special) if special else None,
                                     self.K, self.dnum, self.device), "fhe_ctx_create")
        mods = (ctypes.c_uint64 * (self.L + self.K))()
        psi = (ctypes.c_uint64 * (self.L + self.K))()
        check(lib.fhe_ctx_moduli(self._ptr, mods, psi), "fhe_ctx_moduli")
        self.moduli = [int(v) for v in mods][: self.L]
        self.special = [int(v) for v in mods][self.L:]
        self.psi = [int(v) for v in psi]

    # -- lifetime
    def close(self):
        if getattr(self, "_ptr", None) and self._ptr.value:
            load().fhe_ctx_destroy(self._ptr)
            self._ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._ptr

    @property
    def all_moduli(self):
        return self.moduli + self.special

    def _dev(self):
        return torch.device("cuda", self.device)

    def empty(self, *shape):
        return _empty(shape, dtype=torch.int64, device=self._dev())

    def workspace(self, nbytes: int):
        return _empty((max(int(nbytes), 8) + 7) // 8, dtype=torch.int64, device=self._dev())

    # -- NTT (replaces NTT / iNTT, arithmetic.py:15-19)
    def ntt_(self, t, limb0: int = 0):
        """In-place forward NTT of a [..., nlimbs, N] tensor (limb l uses modulus limb0 + l)."""
        return self._ntt(t, limb0, True)

    def intt_(self, t, limb0: int = 0):
        return self._ntt(t, limb0, False)

    def ntt(self, t, out=None, limb0: int = 0):
        """Out-of-place forward NTT: returns out = NTT(t) (a new tensor unless `out` is given);
        t is left untouched and nothing is copied (the first pass reads t, writes out)."""
        return self._ntt_to(t, out, limb0, True)

    def intt(self, t, out=None, limb0: int = 0):
        return self._ntt_to(t, out, limb0, False)

    def _ntt_to(self, t, out, limb0, fwd):
        _check_tensor(t, "ntt", (self.n,))
        if out is None:
            out = _empty_like(t)
        else:
            _check_out(out, t, t.shape, "ntt: out")
        nl = t.shape[-2] if t.dim() >= 2 else 1
        polys = t.numel() // (nl * self.n)
        fn = load().fhe_ntt_fwd_to if fwd else load().fhe_ntt_inv_to
        with torch.cuda.device(self.device):
            check(fn(self._ptr, _ptr(out), _ptr(t), polys, limb0, nl, _stream(t)), fn.__name__)
        return out

    def _ntt(self, t, limb0, fwd):
        _check_tensor(t, "ntt", (self.n,))
        nl = t.shape[-2] if t.dim() >= 2 else 1
        polys = t.numel() // (nl * self.n)
        fn = load().fhe_ntt_fwd if fwd else load().fhe_ntt_inv
        with torch.cuda.device(self.device):
            check(fn(self._ptr, _ptr(t), polys, limb0, nl, _stream(t)), fn.__name__)
        return t

    # -- coefficient-wise ops (replace vec_add / vec_sub / vec_mul, arithmetic.py:3-13)
    def vec(self, op: str, a, b, out=None, limb0: int = 0):
        _check_tensor(a, op, (self.n,))
        _check_tensor(b, op, (self.n,))
        if a.shape != b.shape:
            raise AssertionError("a.shape != b.shape")  # the reference asserts (arithmetic.py:4)
        out = _empty_like(a) if out is None else _check_out(out, a, a.shape, op + ": out")
        nl = a.shape[-2] if a.dim() >= 2 else 1
        polys = a.numel() // (nl * self.n)
        fn = {"add": load().fhe_vec_add, "sub": load().fhe_vec_sub, "mul": load().fhe_vec_mul}[op]
        with torch.cuda.device(self.device):
            check(fn(self._ptr, _ptr(out), _ptr(a), _ptr(b), polys, limb0, nl, _stream(a)),
                  fn.__name__)
        return out

    # -- HomMult (SURVEY.md §8a')
    def hommult(self, a, b, out=None, limb0: int = 0, workspace=None):
        """a, b: [batch, 2, nlimbs, N] (or [2, nlimbs, N]) coefficient form -> [batch, 3, nlimbs, N]."""
        _check_tensor(a, "hommult", (self.n,))
        _check_tensor(b, "hommult", (self.n,))
        if a.shape != b.shape or a.shape[-3] != 2:
            raise ValueError("hommult: a, b must both be [batch, 2, nlimbs, N]")
        squeeze = a.dim() == 3
        batch = 1 if squeeze else a.shape[0]
        nl = a.shape[-2]
        shape = (3, nl, self.n) if squeeze else (batch, 3, nl, self.n)
        out = self.empty(*shape) if out is None else _check_out(out, a, shape, "hommult: out")
        lib = load()
        ws = workspace
        if ws is None:
            ws = self.workspace(lib.fhe_hommult_workspace(self._ptr, batch, nl))
        with torch.cuda.device(self.device):
            check(lib.fhe_hommult(self._ptr, _ptr(out), _ptr(a), _ptr(b), batch, limb0, nl,
                                  _ptr(ws), _stream(a)), "fhe_hommult")
        return out

    # -- base conversion / key-switch (SURVEY.md §8a')
    def baseconv(self, x, s0: int, t0: int, T: int):
        _check_tensor(x, "baseconv", (self.n,))
        S = x.shape[-2]
        out = self.empty(T, self.n)
        with torch.cuda.device(self.device):
            check(load().fhe_baseconv(self._ptr, _ptr(out), _ptr(x), s0, S, t0, T, _stream(x)),
                  "fhe_baseconv")
        return out

    def _level(self, t, who):
        """The level of t [..., l, N]: its number of Q-limbs l, 1 <= l <= L."""
        lv = t.shape[-2]
        if not 1 <= lv <= self.L:
            raise ValueError(f"{who}: {lv} limbs, expected 1 .. L = {self.L}")
        return lv

    def keyswitch(self, d2, evk_b, evk_a, workspace=None, out=None):
        """d2 [l, N] or [batch, l, N] NTT form over the first l Q-limbs (1 <= l <= L: the level is
        taken from the shape); evk_b/evk_a [dnum, L + K, N] NTT form, the top-level key at every
        level (one key for the whole batch) -> (ks0, ks1) shaped like d2, NTT form.
        out = (ks0, ks1): caller-provided outputs shaped like d2 (either may be d2 itself, in place;
        any other overlap with d2 or between them raises FheError, fhecore.h)."""
        for t, nm in ((d2, "d2"), (evk_b, "evk_b"), (evk_a, "evk_a")):
            _check_tensor(t, nm, (self.n,))
        if tuple(evk_b.shape) != (self.dnum, self.L + self.K, self.n) or evk_a.shape != evk_b.shape:
            raise ValueError("keyswitch: evk must be [dnum, L + K, N]")
        if d2.dim() < 2:
            raise ValueError("keyswitch: d2 must be [..., l, N]")
        lv = self._level(d2, "keyswitch: d2")
        batch = d2.numel() // (lv * self.n)
        if out is None:
            ks0, ks1 = _empty_like(d2), _empty_like(d2)
        else:
            ks0 = _check_out(out[0], d2, d2.shape, "keyswitch: ks0")
            ks1 = _check_out(out[1], d2, d2.shape, "keyswitch: ks1")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_keyswitch_workspace(self._ptr, self.L,
                                        lib.fhe_keyswitch_pass_batch(self._ptr, batch)))
        with torch.cuda.device(self.device):
            check(lib.fhe_keyswitch_level(self._ptr, _ptr(ks0), _ptr(ks1), _ptr(d2), _ptr(evk_b),
                                          _ptr(evk_a), lv, batch, _ptr(ws), _stream(d2)),
                  "fhe_keyswitch_level")
        return ks0, ks1

    # ---- rescale and rotation -------------------------------------
    def galois_elt(self, step: int) -> int:
        """Galois element of a slot rotation by `step` (5^step mod 2N; negative steps invert)."""
        two_n = 2 * self.n
        return pow(5, step, two_n) if step >= 0 else pow(pow(5, -step, two_n), -1, two_n)

    def rescale(self, x, ntt_form: bool = True, workspace=None):
        """Divide-and-round by the last modulus: x [..., l, N] over Q-limbs 0..l-1 (2 <= l <= L)
        -> [..., l - 1, N], same form (oracle: pyoracle.rescale_ntt/_coeff)."""
        _check_tensor(x, "x", (self.n,))
        nl = x.shape[-2]
        polys = x.numel() // (nl * self.n)
        out = _empty(*x.shape[:-2], nl - 1, self.n, dtype=x.dtype, device=x.device)
        lib = load()
        ws = None
        if ntt_form:
            ws = workspace if workspace is not None else self.workspace(
                lib.fhe_rescale_workspace(self._ptr, polys, nl))
        with torch.cuda.device(self.device):
            check(lib.fhe_rescale(self._ptr, _ptr(out), _ptr(x), polys, nl, int(ntt_form),
                                  _ptr(ws), _stream(x)), "fhe_rescale")
        return out

    def automorphism(self, x, galois_elt: int, ntt_form: bool = True, limb0: int = 0):
        """sigma_k(a)(X) = a(X^k) on x [..., nlimbs, N] over limbs [limb0, limb0 + nlimbs)."""
        _check_tensor(x, "x", (self.n,))
        nl = x.shape[-2]
        polys = x.numel() // (nl * self.n)
        out = _empty_like(x)
        with torch.cuda.device(self.device):
            check(load().fhe_automorphism(self._ptr, _ptr(out), _ptr(x), polys, limb0, nl,
                                          galois_elt, int(ntt_form), _stream(x)), "fhe_automorphism")
        return out

    def rotate(self, ct, galois_elt: int, rot_b, rot_a, workspace=None, out=None):
        """ct [..., 2, l, N] NTT form (1 <= l <= L, the level taken from the shape) ->
        (sigma c0 + KS0(sigma c1), KS1(sigma c1)) with the key-switch key rot_b/rot_a
        [dnum, L + K, N] from sigma_k(s) to s, the top-level key at every level.  out: a
        caller-provided output shaped like ct, which must not overlap ct (FheError otherwise,
        fhecore.h)."""
        _check_tensor(ct, "ct", (self.n,))
        if ct.dim() < 3 or ct.shape[-3] != 2:
            raise ValueError("rotate: ct must be [..., 2, l, N]")
        lv = self._level(ct, "rotate: ct")
        if tuple(rot_b.shape) != (self.dnum, self.L + self.K, self.n) or rot_a.shape != rot_b.shape:
            raise ValueError("rotate: key must be [dnum, L + K, N]")
        batch = ct.numel() // (2 * lv * self.n)
        out = _empty_like(ct) if out is None else _check_out(out, ct, ct.shape, "rotate: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_rotate_workspace(self._ptr, lib.fhe_keyswitch_pass_batch(self._ptr, batch)))
        with torch.cuda.device(self.device):
            check(lib.fhe_rotate_level(self._ptr, _ptr(out), _ptr(ct), galois_elt, _ptr(rot_b),
                                       _ptr(rot_a), lv, batch, _ptr(ws), _stream(ct)),
                  "fhe_rotate_level")
        return out

    def rotate_hoisted(self, ct, galois_elts, rot_keys, workspace=None, out=None):
        """Several rotations of the same ct [..., 2, l, N] (NTT form, 1 <= l <= L: the level is
        taken from the shape) sharing one ModUp (fhe_rotate_hoisted): galois_elts[r] with
        rot_keys[r] = (rot_b, rot_a), each [dnum, L + K, N], the top-level key at every level.
        Returns [count, ..., 2, l, N]; output r decrypts to sigma_r(m)."""
        lv = self._ct_level(ct, "rotate_hoisted")
        elts = [int(g) for g in galois_elts]
        g_arr, b_arr, a_arr = self._rot_keys(elts, rot_keys, ct, "rotate_hoisted", keyless=False)
        batch = ct.numel() // (2 * lv * self.n)
        count = len(elts)
        if out is None:
            out = _empty(count, *ct.shape, dtype=ct.dtype, device=ct.device)
        else:
            _check_out(out, ct, (count, *ct.shape), "rotate_hoisted: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_rotate_hoisted_workspace(self._ptr, batch))
        with torch.cuda.device(self.device):
            check(lib.fhe_rotate_hoisted_level(self._ptr, _ptr(out), _ptr(ct), g_arr, b_arr, a_arr,
                                               lv, count, batch, _ptr(ws), _stream(ct)),
                  "fhe_rotate_hoisted_level")
        return out

    def rotate_sum_hoisted(self, ct, galois_elts, rot_keys, pts, workspace=None, out=None):
        """sum_r pts[r] * rot_{galois_elts[r]}(ct) for ct [..., 2, l, N] (NTT form, 1 <= l <= L:
        the level is taken from the shape) with one ModUp and one ModDown (fhe_rotate_sum_hoisted,
        double hoisting): rot_keys[r] = (rot_b, rot_a) [dnum, L + K, N], or None for the unrotated
        term (Galois element 1); pts[r] [L + K, N] NTT form over Q u P.  Keys and plaintexts are
        the top-level ones at every level, read in place.  Returns [..., 2, l, N]."""
        lv = self._ct_level(ct, "rotate_sum_hoisted")
        elts = [int(g) for g in galois_elts]
        count = len(elts)
        if len(pts) != count:
            raise ValueError("rotate_sum_hoisted: one plaintext per term")
        g_arr, b_arr, a_arr = self._rot_keys(elts, rot_keys, ct, "rotate_sum_hoisted")
        p_arr = self._pts(pts, ct, "rotate_sum_hoisted")
        batch = ct.numel() // (2 * lv * self.n)
        out = _empty_like(ct) if out is None else _check_out(out, ct, ct.shape,
                                                             "rotate_sum_hoisted: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_rotate_sum_hoisted_workspace(self._ptr, batch))
        with torch.cuda.device(self.device):
            check(lib.fhe_rotate_sum_hoisted_level(self._ptr, _ptr(out), _ptr(ct), g_arr, b_arr,
                                                   a_arr, p_arr, lv, count, batch, _ptr(ws),
                                                   _stream(ct)), "fhe_rotate_sum_hoisted_level")
        return out

    def _ct_level(self, ct, who):
        """The level of a ciphertext [..., 2, l, N] of the hoisted rotations and rotation sums."""
        _check_tensor(ct, "ct", (self.n,))
        if ct.dim() < 3 or ct.shape[-3] != 2:
            raise ValueError(f"{who}: ct must be [..., 2, l, N]")
        return self._level(ct, f"{who}: ct")

    def _rot_keys(self, elts, rot_keys, ct, who, keyless=True):
        """Host arrays of Galois elements and key pointers, shapes checked.  keyless: the
        unrotated element 1 takes None for a key (rotate_hoisted needs one for every element)."""
        if len(rot_keys) != len(elts):
            raise ValueError(f"{who}: one key{' (or None)' if keyless else ''} per Galois element")
        for g, key in zip(elts, rot_keys):
            if key is None:
                if g != 1 or not keyless:
                    raise ValueError(f"{who}: only Galois element 1 takes no key" if keyless else
                                     f"{who}: every Galois element takes a key")
                continue
            kb, ka = key
            if tuple(kb.shape) != (self.dnum, self.L + self.K, self.n) or ka.shape != kb.shape:
                raise ValueError(f"{who}: keys must be [dnum, L + K, N]")
            if kb.device != ct.device or ka.device != ct.device or not (
                    kb.is_contiguous() and ka.is_contiguous()):
                raise ValueError(f"{who}: keys must be contiguous on the ct's device")
        k = max(len(elts), 1)
        return ((ctypes.c_uint32 * k)(*elts),
                (ctypes.c_void_p * k)(*[kk[0].data_ptr() if kk else None for kk in rot_keys]),
                (ctypes.c_void_p * k)(*[kk[1].data_ptr() if kk else None for kk in rot_keys]))

    def _pts(self, pts, ct, who):
        for pt in pts:
            if tuple(pt.shape) != (self.L + self.K, self.n) or pt.device != ct.device or not \
                    pt.is_contiguous():
                raise ValueError(f"{who}: plaintexts must be contiguous [L + K, N] on the ct's "
                                 "device")
        return (ctypes.c_void_p * max(len(pts), 1))(*[p.data_ptr() for p in pts])

    def rotate_sum_multi(self, cts, galois_elts, rot_keys, workspace=None, out=None):
        """sum_r rot_{galois_elts[r]}(cts[r]) over different ciphertexts (each [..., 2, l, N], NTT
        form, one shape, 1 <= l <= L: the level is taken from it) with one ModDown (fhe_rotate_sum_multi, the giant-step sum of a BSGS
        linear transform); rot_keys[r] = (rot_b, rot_a) or None for Galois element 1."""
        if not cts:
            raise ValueError("rotate_sum_multi: at least one ciphertext")
        ct = cts[0]
        lv = self._ct_level(ct, "rotate_sum_multi")
        for c in cts:
            if c.shape != ct.shape or c.device != ct.device or not c.is_contiguous():
                raise ValueError("rotate_sum_multi: ciphertexts of one shape, contiguous, on one "
                                 "device")
        elts = [int(g) for g in galois_elts]
        if len(cts) != len(elts):
            raise ValueError("rotate_sum_multi: one Galois element per ciphertext")
        g_arr, b_arr, a_arr = self._rot_keys(elts, rot_keys, ct, "rotate_sum_multi")
        batch = ct.numel() // (2 * lv * self.n)
        out = _empty_like(ct) if out is None else _check_out(out, ct, ct.shape,
                                                             "rotate_sum_multi: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_rotate_sum_multi_workspace(self._ptr, len(cts), batch))
        c_arr = (ctypes.c_void_p * len(cts))(*[c.data_ptr() for c in cts])
        with torch.cuda.device(self.device):
            check(lib.fhe_rotate_sum_multi_level(self._ptr, _ptr(out), c_arr, g_arr, b_arr, a_arr,
                                                 lv, len(elts), batch, _ptr(ws), _stream(ct)),
                  "fhe_rotate_sum_multi_level")
        return out

    def linear_transform(self, ct, baby_elts, baby_keys, giant_elts, giant_keys, pts,
                         workspace=None, out=None):
        """Baby-step / giant-step plaintext-matrix product with both hoistings
        (fhe_linear_transform): sum_g rot_{giant[g]}(sum_b pts[g][b] rot_{baby[b]}(ct)) for
        ct [..., 2, l, N] NTT form (1 <= l <= L: the level is taken from the shape); pts[g][b]
        [L + K, N] NTT form over Q u P and the keys [dnum, L + K, N], the top-level ones at every
        level."""
        lv = self._ct_level(ct, "linear_transform")
        baby = [int(g) for g in baby_elts]
        giant = [int(g) for g in giant_elts]
        n1, n2 = len(baby), len(giant)
        if len(pts) != n2 or any(len(row) != n1 for row in pts):
            raise ValueError("linear_transform: pts must be n2 lists of n1 plaintexts")
        bg, bb, ba = self._rot_keys(baby, baby_keys, ct, "linear_transform")
        gg, gb, ga = self._rot_keys(giant, giant_keys, ct, "linear_transform")
        p_arr = self._pts([p for row in pts for p in row], ct, "linear_transform")
        batch = ct.numel() // (2 * lv * self.n)
        out = _empty_like(ct) if out is None else _check_out(out, ct, ct.shape,
                                                             "linear_transform: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_linear_transform_workspace(self._ptr, n2, batch))
        with torch.cuda.device(self.device):
            check(lib.fhe_linear_transform_level(self._ptr, _ptr(out), _ptr(ct), n1, n2, bg, bb, ba,
                                                 gg, gb, ga, p_arr, lv, batch, _ptr(ws),
                                                 _stream(ct)), "fhe_linear_transform_level")
        return out

    # ---- sampling, keys, encryption --------------------------------
    # seed=None draws a fresh 64-bit nonce from the OS CSPRNG.  An explicit seed is for
    # reproducible tests: never reuse one per secret key (fhecore.h SECURITY note).
    KIND = {"uniform": 0, "ternary": 1, "error": 2}

    def sample(self, kind: str, polys: int, seed: int, tag: int, limb0: int = 0, nlimbs=None):
        """[polys, nlimbs, N] residues of a Philox4x32-10 draw (oracle: pyoracle.sample)."""
        nl = (self.L + self.K - limb0) if nlimbs is None else nlimbs
        out = _empty(polys, nl, self.n, dtype=torch.int64, device=self._dev())
        with torch.cuda.device(self.device):
            check(load().fhe_sample(self._ptr, _ptr(out), polys, limb0, nl, self.KIND[kind],
                                    seed, tag, _stream(out)), "fhe_sample")
        return out

    def keygen_secret(self, seed=None, hamming_weight=None):
        """Ternary secret, NTT form over all L + K limbs: [L + K, N].  hamming_weight = h: exactly
        h coefficients are +-1 (fhe_keygen_secret_sparse; the secret of fhecore.bootstrap)."""
        seed = _nonce(seed)
        sk = _empty(self.L + self.K, self.n, dtype=torch.int64, device=self._dev())
        with torch.cuda.device(self.device):
            if hamming_weight is None:
                check(load().fhe_keygen_secret(self._ptr, _ptr(sk), seed, _stream(sk)),
                      "fhe_keygen_secret")
            else:
                h = int(hamming_weight)
                if not 0 <= h < 1 << 32:  # (the range [1, N] is fhe_keygen_secret_sparse's check)
                    raise ValueError("keygen_secret: hamming_weight out of range")
                check(load().fhe_keygen_secret_sparse(self._ptr, _ptr(sk), h, seed, _stream(sk)),
                      "fhe_keygen_secret_sparse")
        return sk

    def keygen_public(self, sk, seed=None):
        seed = _nonce(seed)
        pk = _empty(2, self.L, self.n, dtype=torch.int64, device=self._dev())
        with torch.cuda.device(self.device):
            check(load().fhe_keygen_public(self._ptr, _ptr(pk), _ptr(sk), seed, _stream(pk)),
                  "fhe_keygen_public")
        return pk

    def keygen_switch(self, sk, s_from, seed=None):
        """Key-switch key from s_from ([L + K, N] NTT form) to sk: (evk_b, evk_a), each
        [dnum, L + K, N] -- the operands of keyswitch / rotate / mul_relin."""
        seed = _nonce(seed)
        key = _empty(2, self.dnum, self.L + self.K, self.n, dtype=torch.int64, device=self._dev())
        with torch.cuda.device(self.device):
            check(load().fhe_keygen_switch(self._ptr, _ptr(key), _ptr(sk), _ptr(s_from), seed,
                                           _stream(key)), "fhe_keygen_switch")
        return key[0], key[1]

    def keygen_relin(self, sk, seed=None):
        """Relinearisation key: switches s^2 to s."""
        s2 = _empty_like(sk)
        lib = load()
        with torch.cuda.device(self.device):
            check(lib.fhe_vec_mul(self._ptr, _ptr(s2), _ptr(sk), _ptr(sk), 1, 0, self.L + self.K,
                                  _stream(sk)), "fhe_vec_mul")
        return self.keygen_switch(sk, s2, seed)

    def keygen_rotation(self, sk, galois_elt: int, seed=None):
        """Rotation key for Galois element k: switches sigma_k(s) to s."""
        return self.keygen_switch(sk, self.automorphism(sk, galois_elt, ntt_form=True), seed)

    def encrypt(self, pt, pk, seed=None, *, level=None, batch=None, index0=0, workspace=None,
                out=None):
        """Public-key encryption of NTT-form plaintexts.  A [L, N] plaintext with no keyword
        argument is the single top-level call (fhe_encrypt) -> [2, L, N].  Anything else is the
        batched call (fhe_encrypt_level): pt [..., rows, N] (one plaintext per ciphertext),
        [rows, N] with batch= (one plaintext for the whole batch) or None (zero; batch= says how
        many), rows >= level (default: min(rows, L)) read in place -> [..., 2, level, N].
        Ciphertext i draws with the nonce (seed, index0 + i): one seed serves a stream of batches,
        and a (seed, index) pair must never repeat under one key (fhecore.h SECURITY note).
        workspace: fhe_encrypt_workspace(ctx, level, batch) bytes; out must not overlap pt, the
        key or the workspace."""
        return self._encrypt(pt, pk, False, seed, level, batch, index0, workspace, out)

    def encrypt_sk(self, pt, sk, seed=None, *, level=None, batch=None, index0=0, workspace=None,
                   out=None):
        """Secret-key encryption (c1 uniform, c0 = e - c1 s + pt); the arguments of encrypt, the
        batched call being fhe_encrypt_sk_level."""
        return self._encrypt(pt, sk, True, seed, level, batch, index0, workspace, out)

    def _encrypt(self, pt, key, secret, seed, level, batch, index0, workspace, out):
        who = "encrypt_sk" if secret else "encrypt"
        seed = _nonce(seed)
        lib = load()
        if (pt is not None and pt.dim() == 2 and pt.shape[0] == self.L and level is None and
                batch is None and index0 == 0 and workspace is None and out is None):
            ct = _empty(2, self.L, self.n, dtype=torch.int64, device=self._dev())
            with torch.cuda.device(self.device):
                if secret:
                    check(lib.fhe_encrypt_sk(self._ptr, _ptr(ct), _ptr(pt), _ptr(key), seed,
                                             _stream(ct)), "fhe_encrypt_sk")
                else:
                    ws = self.workspace(self.L * self.n * 8)  # a Graph keeps it
                    check(lib.fhe_encrypt(self._ptr, _ptr(ct), _ptr(pt), _ptr(key), seed, _ptr(ws),
                                          _stream(ct)), "fhe_encrypt")
            return ct
        _check_tensor(key, f"{who}: key", (self.n,))
        rows, pt_batch = 0, 1
        lead = () if batch is None else (int(batch),)
        if pt is not None:
            _check_tensor(pt, f"{who}: pt", (self.n,))
            if pt.dim() < 2 or pt.device != key.device:
                raise ValueError(f"{who}: pt must be [rows, N] or [..., rows, N] on the key's device")
            rows = pt.shape[-2]
            if pt.dim() > 2:
                lead = tuple(pt.shape[:-2])
                pt_batch = pt.numel() // (rows * self.n)
                if batch is not None and int(batch) != pt_batch:
                    raise ValueError(f"{who}: batch={batch} but pt holds {pt_batch} plaintexts")
        count = int(np.prod(lead, dtype=np.int64)) if lead else 1
        if pt is not None and pt.dim() > 2:
            pt_batch = count
        if level is None:
            level = self.L if pt is None else min(rows, self.L)
        level = int(level)
        if not 1 <= level <= self.L:
            raise ValueError(f"{who}: level must be in [1, {self.L}]")
        if not 0 <= int(index0) < 1 << 32:
            raise ValueError(f"{who}: index0 out of range")
        shape = (*lead, 2, level, self.n)
        if out is None:
            out = _empty(shape, dtype=torch.int64, device=key.device)
        else:
            _check_out(out, key, shape, f"{who}: out")
        fn = lib.fhe_encrypt_sk_level if secret else lib.fhe_encrypt_level
        with torch.cuda.device(self.device):
            ws = workspace if workspace is not None else self.workspace(
                lib.fhe_encrypt_workspace(self._ptr, level, count))
            check(fn(self._ptr, _ptr(out), _ptr(pt), rows, pt_batch, _ptr(key), level, count, seed,
                     int(index0), _ptr(ws), _stream(out)),
                  "fhe_encrypt_sk_level" if secret else "fhe_encrypt_level")
        return out

    def encrypt_slots(self, z, delta, key, *, secret=False, level=None, log_slots=None, seed=None,
                      index0=0, workspace=None, out=None):
        """z complex128 [..., 2^log_slots] (default: N/2, full packing) -> ciphertexts
        [..., 2, level, N] (default level: L) in one call (fhe_encrypt_slots): bit for bit
        encrypt(encode(z, delta, level, log_slots=log_slots), key, ...) (encrypt_sk with
        secret=True, key then being sk), without forming the plaintext: the message's coefficients
        join the error before the transform.  seed, index0, workspace, out as encrypt."""
        ls, ns = self._log_slots(log_slots, "encrypt_slots")
        z = self._slots(z, "encrypt_slots", ns)
        _check_tensor(key, "encrypt_slots: key", (self.n,))
        seed = _nonce(seed)
        level = self.L if level is None else int(level)
        if not 1 <= level <= self.L:
            raise ValueError(f"encrypt_slots: level must be in [1, {self.L}]")
        if not 0 <= int(index0) < 1 << 32:
            raise ValueError("encrypt_slots: index0 out of range")
        count = z.numel() // ns
        shape = (*z.shape[:-1], 2, level, self.n)
        if out is None:
            out = _empty(shape, dtype=torch.int64, device=z.device)
        else:
            _check_out(out, z, shape, "encrypt_slots: out")
        lib = load()
        with torch.cuda.device(self.device):
            ws = workspace if workspace is not None else self.workspace(
                lib.fhe_encrypt_workspace(self._ptr, level, count))
            check(lib.fhe_encrypt_slots(self._ptr, _ptr(out), _ptr(z), float(delta), ls, _ptr(key),
                                        int(bool(secret)), level, count, seed, int(index0), _ptr(ws),
                                        _stream(out)), "fhe_encrypt_slots")
        return out

    def decrypt(self, ct, sk):
        """ct [..., 2, l, N] (any level l <= L) -> plaintext c0 + c1 s [..., l, N], NTT form."""
        _check_tensor(ct, "ct", (self.n,))
        nl = ct.shape[-2]
        batch = ct.numel() // (2 * nl * self.n)
        pt = _empty(*ct.shape[:-3], nl, self.n, dtype=ct.dtype, device=ct.device)
        with torch.cuda.device(self.device):
            check(load().fhe_decrypt(self._ptr, _ptr(pt), _ptr(ct), _ptr(sk), batch, nl, _stream(ct)),
                  "fhe_decrypt")
        return pt

    # ---- fused multiply -> relinearise -> rescale ------------------
    def mul_relin(self, a, b, evk_b, evk_a, rescale: bool = True, workspace=None, out=None):
        """a, b [..., 2, l, N] NTT form (1 <= l <= L, the level taken from the shape) ->
        Relin(a x b) [..., 2, l, N] (rescale: [..., 2, l-1, N], needs l >= 2), NTT form; evk_b /
        evk_a [dnum, L + K, N], the top-level key at every level (oracle: pyoracle.mul_relin)."""
        _check_tensor(a, "a", (self.n,))
        _check_tensor(b, "b", (self.n,))
        if a.shape != b.shape or a.dim() < 3 or a.shape[-3] != 2:
            raise ValueError("mul_relin: a and b must both be [..., 2, l, N]")
        lv = self._level(a, "mul_relin: a")
        if tuple(evk_b.shape) != (self.dnum, self.L + self.K, self.n) or evk_a.shape != evk_b.shape:
            raise ValueError("mul_relin: key must be [dnum, L + K, N]")
        batch = a.numel() // (2 * lv * self.n)
        shape = (*a.shape[:-2], lv - (1 if rescale else 0), self.n)
        if out is None:
            out = _empty(shape, dtype=a.dtype, device=a.device)
        else:
            _check_out(out, a, shape, "mul_relin: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_mul_relin_workspace(self._ptr, lib.fhe_keyswitch_pass_batch(self._ptr, batch)))
        with torch.cuda.device(self.device):
            check(lib.fhe_mul_relin_level(self._ptr, _ptr(out), _ptr(a), _ptr(b), _ptr(evk_b),
                                          _ptr(evk_a), lv, batch, int(rescale), _ptr(ws),
                                          _stream(a)), "fhe_mul_relin_level")
        return out

    def mul_sum_relin(self, a_list, b_list, evk_b, evk_a, rescale: bool = True, level=None,
                      workspace=None, out=None):
        """[rescale]( Relin( sum_i a_list[i] x b_list[i] ) ) with one key-switch and one rescale
        whatever the number of terms (fhe_mul_sum_relin_level; up to 16 terms).  Every operand
        [..., 2, l, N] NTT form with one leading (batch) shape and any level l >= level (default:
        the lowest of them), cut to `level` limbs on the fly; operands may be one tensor (squares,
        a shared factor).  Returns [..., 2, level, N], or with rescale [..., 2, level - 1, N]; out
        must not overlap an operand.  workspace: fhe_mul_relin_workspace(ctx, pass) bytes; None
        takes the context's internal one, which is refused while a Graph is capturing."""
        if not a_list or len(a_list) != len(b_list):
            raise ValueError("mul_sum_relin: two lists of one length, at least one term")
        la = [self._ct_level(c, "mul_sum_relin") for c in a_list]
        lb = [self._ct_level(c, "mul_sum_relin") for c in b_list]
        ref = a_list[0]
        lead = tuple(ref.shape[:-3])
        for c in (*a_list, *b_list):
            if tuple(c.shape[:-3]) != lead or c.device != ref.device:
                raise ValueError("mul_sum_relin: ciphertexts of one batch shape on one device")
        if tuple(evk_b.shape) != (self.dnum, self.L + self.K, self.n) or evk_a.shape != evk_b.shape:
            raise ValueError("mul_sum_relin: key must be [dnum, L + K, N]")
        level = min(la + lb) if level is None else int(level)
        count = len(a_list)
        batch = ref.numel() // (2 * la[0] * self.n)
        shape = (*lead, 2, level - (1 if rescale else 0), self.n)
        if out is None:
            out = _empty(shape, dtype=ref.dtype, device=ref.device)
        else:
            _check_out(out, ref, shape, "mul_sum_relin: out")
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_mul_relin_workspace(self._ptr, lib.fhe_keyswitch_pass_batch(self._ptr, batch)))
        a_arr = (ctypes.c_void_p * count)(*[c.data_ptr() for c in a_list])
        b_arr = (ctypes.c_void_p * count)(*[c.data_ptr() for c in b_list])
        la_arr = (ctypes.c_uint32 * count)(*la)
        lb_arr = (ctypes.c_uint32 * count)(*lb)
        with torch.cuda.device(self.device):
            check(lib.fhe_mul_sum_relin_level(self._ptr, _ptr(out), a_arr, la_arr, b_arr, lb_arr,
                                              _ptr(evk_b), _ptr(evk_a), level, count, batch,
                                              int(rescale), _ptr(ws), _stream(ref)),
                  "fhe_mul_sum_relin_level")
        return out

    # ---- plaintext arithmetic at any level (fhe_lincomb_level / fhe_mul_plain_level) --------
    def encode_scalars(self, values, delta=1.0, exact: bool = False):
        """Device table [len(values), L] of round(v * delta) mod q_j (Python integers, negative
        values wrap): the `scalars` of lincomb, one row per term, encoded once over all L limbs
        and read at every level.  exact=True: the values are already integers."""
        if exact:
            ints = [int(v) for v in values]
        else:
            d = Fraction(delta)
            ints = [int(round(Fraction(v) * d)) for v in values]
        tab = np.array([[k % q for q in self.moduli] for k in ints], dtype=np.uint64)
        return to_device(tab.reshape(len(ints), self.L), self._dev())

    def lincomb(self, cts, scalars, const: bool = False, rescale: bool = False, level=None,
                workspace=None, out=None):
        """[rescale]( sum_i scalars[i] * cts[i] (+ scalars[len(cts)] on every slot of c0) ) in one
        pass (fhe_lincomb_level).  cts[i] [..., 2, l_i, N] NTT form with one leading (batch) shape
        and any levels l_i >= level (default: the lowest of them): a higher term is cut to `level`
        limbs on the fly.  scalars: a device table [rows >= len(cts) (+ 1 with const), >= level]
        (encode_scalars).  Returns [..., 2, level, N], or with rescale [..., 2, level - 1, N].
        out may be one of the cts at that level when rescale is off.  workspace (rescale only):
        fhe_lincomb_workspace(ctx, batch) bytes; None takes the context's internal one, which is
        refused while a Graph is capturing."""
        if not cts:
            raise ValueError("lincomb: at least one ciphertext")
        lvs = [self._ct_level(c, "lincomb") for c in cts]
        ref = cts[0]
        lead = tuple(ref.shape[:-3])
        for c in cts:
            if tuple(c.shape[:-3]) != lead or c.device != ref.device:
                raise ValueError("lincomb: ciphertexts of one batch shape on one device")
        level = min(lvs) if level is None else int(level)
        count = len(cts)
        _check_tensor(scalars, "lincomb: scalars")
        if scalars.dim() != 2 or scalars.shape[0] < count + (1 if const else 0) or \
                scalars.device != ref.device:
            raise ValueError("lincomb: scalars must be a device table [len(cts) (+ 1), stride]")
        batch = ref.numel() // (2 * lvs[0] * self.n)
        shape = (*lead, 2, level - (1 if rescale else 0), self.n)
        if out is None:
            out = _empty(shape, dtype=ref.dtype, device=ref.device)
        else:
            _check_out(out, ref, shape, "lincomb: out")
        c_arr = (ctypes.c_void_p * count)(*[c.data_ptr() for c in cts])
        l_arr = (ctypes.c_uint32 * count)(*lvs)
        with torch.cuda.device(self.device):
            check(load().fhe_lincomb_level(self._ptr, _ptr(out), c_arr, l_arr, _ptr(scalars),
                                           scalars.shape[1], int(const), level, count, batch,
                                           int(rescale), _ptr(workspace), _stream(ref)),
                  "fhe_lincomb_level")
        return out

    def mul_plain(self, ct, pt, rescale: bool = False, workspace=None, out=None):
        """[rescale]( ct * pt ) (fhe_mul_plain_level): ct [..., 2, l, N] NTT form, pt [rows, N]
        (one plaintext for the whole batch) or [..., rows, N] (one per ciphertext), NTT form,
        rows >= l: a top-level [L, N] plaintext or a diagonal [L + K, N] is read in place at every
        level.  out may be ct when rescale is off; workspace as lincomb."""
        lv = self._ct_level(ct, "mul_plain")
        _check_tensor(pt, "mul_plain: pt", (self.n,))
        lead = tuple(ct.shape[:-3])
        if pt.dim() < 2 or pt.device != ct.device or (
                pt.dim() > 2 and tuple(pt.shape[:-2]) != lead):
            raise ValueError("mul_plain: pt must be [rows, N] or [..., rows, N] with ct's batch "
                             "shape, on ct's device")
        batch = ct.numel() // (2 * lv * self.n)
        shape = (*lead, 2, lv - (1 if rescale else 0), self.n)
        if out is None:
            out = _empty(shape, dtype=ct.dtype, device=ct.device)
        else:
            _check_out(out, ct, shape, "mul_plain: out")
        with torch.cuda.device(self.device):
            check(load().fhe_mul_plain_level(self._ptr, _ptr(out), _ptr(ct), _ptr(pt),
                                             pt.shape[-2], 1 if pt.dim() == 2 else batch, lv,
                                             batch, int(rescale), _ptr(workspace), _stream(ct)),
                  "fhe_mul_plain_level")
        return out

    def drop_level(self, ct, level: int, out=None):
        """ct [..., 2, l, N] -> its first `level` <= l limbs [..., 2, level, N] (dropping RNS limbs
        lowers the level; the scale is unchanged): lincomb with one term and scalar 1."""
        if getattr(self, "_one", None) is None:
            self._one = self.encode_scalars([1], exact=True)
        return self.lincomb([ct], self._one, level=level, out=out)

    # ---- real / imaginary split and merge (fhe_conj_split_level / fhe_conj_merge_level) --------
    def _conj_pair(self, a, b, who):
        lv = self._ct_level(a, who)
        _check_tensor(b, f"{who}: second operand", (self.n,))
        if b.shape != a.shape or b.device != a.device:
            raise ValueError(f"{who}: both operands must be [..., 2, l, N] of one shape on one device")
        return lv, a.numel() // (2 * lv * self.n)

    def conj_split(self, ct, cc, out=None):
        """ct [..., 2, l, N] NTT form and its conjugate cc (rotate by Galois element 2N - 1) ->
        (re, im) = (ct + cc, -X^(N/2) (ct - cc)), whose slots are 2 Re z and 2 Im z: one pass,
        exact, no level consumed.  out = (re, im): caller-provided outputs, each of which may be
        ct or cc itself; no workspace."""
        lv, batch = self._conj_pair(ct, cc, "conj_split")
        if out is None:
            re, im = _empty_like(ct), _empty_like(ct)
        else:
            re = _check_out(out[0], ct, ct.shape, "conj_split: re")
            im = _check_out(out[1], ct, ct.shape, "conj_split: im")
        with torch.cuda.device(self.device):
            check(load().fhe_conj_split_level(self._ptr, _ptr(re), _ptr(im), _ptr(ct), _ptr(cc), lv,
                                              batch, _stream(ct)), "fhe_conj_split_level")
        return re, im

    def conj_merge(self, a, b, out=None):
        """a + X^(N/2) b for a, b [..., 2, l, N] NTT form: slots a_j + i b_j, one pass, exact.
        out may be a or b itself; no workspace."""
        lv, batch = self._conj_pair(a, b, "conj_merge")
        out = _empty_like(a) if out is None else _check_out(out, a, a.shape, "conj_merge: out")
        with torch.cuda.device(self.device):
            check(load().fhe_conj_merge_level(self._ptr, _ptr(out), _ptr(a), _ptr(b), lv, batch,
                                              _stream(a)), "fhe_conj_merge_level")
        return out

    # ---- ModRaise (fhe_mod_raise): from the bottom of the chain back up ---------------------
    def mod_raise(self, ct, level=None, workspace=None, out=None):
        """ct [..., 2, l, N] NTT form at any level l (only limb 0 is read) -> [..., 2, level, N]
        (default: L): the centred lift of limb 0's coefficients reduced modulo every q_j, NTT form.
        Limb 0 of the result is ct's; the result decrypts to m + q_0 I, I a small integer
        polynomial (fhecore.polyeval.eval_mod removes it).  out must not overlap ct.  workspace:
        fhe_mod_raise_workspace(ctx, batch) bytes; None takes the context's internal one, which is
        refused while a Graph is capturing."""
        lv = self._ct_level(ct, "mod_raise")
        level = self.L if level is None else int(level)  # range-checked by fhe_mod_raise
        batch = ct.numel() // (2 * lv * self.n)
        shape = (*ct.shape[:-2], level, self.n)
        if out is None:
            out = _empty(shape, dtype=ct.dtype, device=ct.device)
        else:
            _check_out(out, ct, shape, "mod_raise: out")
        with torch.cuda.device(self.device):
            check(load().fhe_mod_raise(self._ptr, _ptr(out), _ptr(ct), lv, level, batch,
                                       _ptr(workspace), _stream(ct)), "fhe_mod_raise")
        return out

    # ---- CKKS encode / decode on the device (fhe_encode / fhe_decode) -----------------------
    def _log_slots(self, log_slots, who):
        """(log_slots or log_n - 1, the slot count); sparse packing is 0 <= log_slots < log_n - 1."""
        if log_slots is None:
            return self.log_n - 1, self.n // 2
        if not 0 <= int(log_slots) <= self.log_n - 1:
            raise ValueError(f"{who}: log_slots must be in [0, {self.log_n - 1}]")
        return int(log_slots), 1 << int(log_slots)

    def _slots(self, z, who, ns=None):
        ns = self.n // 2 if ns is None else ns
        if not isinstance(z, torch.Tensor):
            z = torch.from_numpy(np.ascontiguousarray(np.asarray(z, dtype=np.complex128)))
        if z.dtype != torch.complex128:
            raise TypeError(f"{who}: expected complex128 slots, got {z.dtype}")
        if z.dim() < 1 or z.shape[-1] != ns:
            raise ValueError(f"{who}: expected [..., {ns}] slots, got {tuple(z.shape)}")
        return z.to(self._dev()).contiguous()

    def encode(self, z, delta, level=None, special=False, workspace=None, out=None,
               log_slots=None):
        """z complex128 [..., N/2] (a host array is moved to the device first) -> the plaintexts
        [..., level (+ K), N] in NTT form (fhe_encode): the inverse special FFT over the rotation
        group, c = rint(v delta / (N/2)), every row the NTT of c modulo its limb -- the Q-limbs
        0 .. level-1 (default L) and, with special, the P-limbs after them.  level = L with special
        is the [L + K, N] diagonal linear_transform / rotate_sum_hoisted read at every level;
        special=False is the [level, N] plaintext of mul_plain / encrypt.  Slot j sits at the root
        exp(i pi 5^j / N) as in fhecore.ckks.Encoder, whose coefficients this differs from by at
        most a unit.  Precondition: |c| < 2^62.  workspace: fhe_encode_workspace(ctx, count) bytes;
        None takes the context's internal one, which is refused while a Graph is capturing.

        log_slots (sparse packing, fhe_encode_sparse): z is [..., 2^log_slots] and the result is,
        bit for bit, the encoding of z tiled N / 2^(log_slots + 1) times: the plaintext of
        Z[Y]/(Y^(2 n_s) + 1), Y = X^gap, with zeros between the multiples of gap.  None is full
        packing (fhe_encode)."""
        ls, ns = self._log_slots(log_slots, "encode")
        z = self._slots(z, "encode", ns)
        level = self.L if level is None else int(level)  # range-checked by fhe_encode
        rows = level + (self.K if special else 0)
        count = z.numel() // ns
        shape = (*z.shape[:-1], rows, self.n)
        if out is None:
            out = _empty(shape, dtype=torch.int64, device=z.device)
        else:
            _check_out(out, z, shape, "encode: out")
        with torch.cuda.device(self.device):
            if log_slots is None:
                check(load().fhe_encode(self._ptr, _ptr(out), _ptr(z), float(delta), level,
                                        int(bool(special)), count, _ptr(workspace), _stream(z)),
                      "fhe_encode")
            else:
                check(load().fhe_encode_sparse(self._ptr, _ptr(out), _ptr(z), float(delta), ls,
                                               level, int(bool(special)), count, _ptr(workspace),
                                               _stream(z)), "fhe_encode_sparse")
        return out

    def decode(self, pt, delta, level=None, workspace=None, out=None, log_slots=None):
        """pt [..., rows, N] NTT form -> complex128 slots [..., N/2] (fhe_decode).  level (default:
        min(rows, L)) says how many Q-limbs pt carries a value over; limb 0 is read, and limb 1 at
        level >= 2, through the rows' own stride (an [L + K, N] diagonal decodes in place).  The
        value is centred over q_0 q_1 (q_0 at level 1), so the plaintext's true centred value must
        be below q_0 q_1 / 2 (q_0 / 2) in magnitude.

        log_slots (sparse packing, fhe_decode_sparse): only the coefficients at the multiples of
        gap = N / 2^(log_slots + 1) are read -- the projection onto the subring, which drops what
        a ciphertext's noise left between them -- and the result is [..., 2^log_slots]."""
        ls, ns = self._log_slots(log_slots, "decode")
        _check_tensor(pt, "decode: pt")
        if pt.dim() < 2 or pt.shape[-1] != self.n:
            raise ValueError(f"decode: expected [..., rows, {self.n}], got {tuple(pt.shape)}")
        rows = pt.shape[-2]
        level = min(rows, self.L) if level is None else int(level)  # range-checked by fhe_decode
        count = pt.numel() // (rows * self.n)
        shape = (*pt.shape[:-2], ns)
        if out is None:
            out = _empty(shape, dtype=torch.complex128, device=pt.device)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.complex128 or \
                    out.device != pt.device or not out.is_contiguous() or \
                    tuple(out.shape) != shape:
                raise ValueError(f"decode: out must be a contiguous complex128 {shape} tensor on "
                                 "pt's device")
        with torch.cuda.device(self.device):
            if log_slots is None:
                check(load().fhe_decode(self._ptr, _ptr(out), _ptr(pt), float(delta), rows, level,
                                        count, _ptr(workspace), _stream(pt)), "fhe_decode")
            else:
                check(load().fhe_decode_sparse(self._ptr, _ptr(out), _ptr(pt), float(delta), ls,
                                               rows, level, count, _ptr(workspace), _stream(pt)),
                      "fhe_decode_sparse")
        return out

    def decrypt_slots(self, ct, sk, delta, *, log_slots=None, workspace=None, out=None):
        """ct [..., 2, level, N] NTT form (the level taken from the shape) -> complex128 slots
        [..., 2^log_slots] (default: N/2, full packing) in one call (fhe_decrypt_slots): bit for
        bit decode(decrypt(ct, sk), delta, level=level, log_slots=log_slots), without forming the
        plaintext: only limb 0 of the ciphertext is read, and limb 1 at level >= 2, and c0 + c1 s
        is computed by the inverse transform's first pass as it loads.  sk is [L + K, N].
        workspace: fhe_decode_workspace(ctx, count) bytes; None takes the context's internal one,
        which is refused while a Graph is capturing.  out as decode."""
        ls, ns = self._log_slots(log_slots, "decrypt_slots")
        _check_tensor(ct, "decrypt_slots: ct", (self.n,))
        _check_tensor(sk, "decrypt_slots: sk", (self.n,))
        if ct.dim() < 3 or ct.shape[-3] != 2:
            raise ValueError(f"decrypt_slots: expected [..., 2, level, {self.n}], got "
                             f"{tuple(ct.shape)}")
        level = ct.shape[-2]
        if not 1 <= level <= self.L:
            raise ValueError(f"decrypt_slots: level must be in [1, {self.L}]")
        if sk.dim() != 2 or sk.shape[0] < min(level, 2) or sk.device != ct.device:
            raise ValueError(f"decrypt_slots: sk must be [L + K, {self.n}] on ct's device")
        count = ct.numel() // (2 * level * self.n)
        shape = (*ct.shape[:-3], ns)
        if out is None:
            out = _empty(shape, dtype=torch.complex128, device=ct.device)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.complex128 or \
                    out.device != ct.device or not out.is_contiguous() or \
                    tuple(out.shape) != shape:
                raise ValueError(f"decrypt_slots: out must be a contiguous complex128 {shape} "
                                 "tensor on ct's device")
        with torch.cuda.device(self.device):
            check(load().fhe_decrypt_slots(self._ptr, _ptr(out), _ptr(ct), _ptr(sk), float(delta),
                                           ls, level, count, _ptr(workspace), _stream(ct)),
                  "fhe_decrypt_slots")
        return out

    def encode_diagonals(self, diags, n1: int, n2: int, delta, level=None, log_slots=None):
        """The plaintexts of a baby-step / giant-step matrix product from a slot matrix's
        diagonals: diags maps k < n1 n2 to the complex [N/2] vector d_k[j] = A[j][(j + k) mod N/2]
        (absent diagonals are zero).  Returns (baby_elts, giant_elts, pts) for linear_transform,
        which then computes A z = sum_k d_k * rot_k(z).

        Direction: rotate by galois_elt(step) moves slot j + step into slot j,
        rot_step(z)[j] = z[(j + step) mod N/2] (numpy: np.roll(z, -step)).  With k = g n1 + b,
        A z = sum_g rot_{g n1}(sum_b rot_{-g n1}(d_k) * rot_b(z)), so pts[g][b] encodes d_k rolled
        towards higher indices by g n1 (torch.roll(d_k, g n1)), over Q u P at scale delta.  All
        n1 n2 encodings are one fhe_encode call.  level is accepted for symmetry with the other
        calls: the plaintexts are the top-level [L + K, N] ones, read in place at every level.
        log_slots: the diagonals are [2^log_slots] vectors of a sparsely packed matrix (encode's
        keyword); the rotation steps are taken on the full ring all the same."""
        if n1 < 1 or n2 < 1:
            raise ValueError("encode_diagonals: n1, n2 >= 1")
        if level is not None and not 1 <= int(level) <= self.L:
            raise ValueError("encode_diagonals: level must be in [1, L]")
        _, ns = self._log_slots(log_slots, "encode_diagonals")
        bad = [k for k in diags if not 0 <= int(k) < n1 * n2]
        if bad:
            raise ValueError(f"encode_diagonals: diagonal indices {bad} outside [0, n1 n2)")
        z = torch.zeros(n2, n1, ns, dtype=torch.complex128, device=self._dev())
        for k, d in diags.items():
            g, b = divmod(int(k), n1)
            z[g, b] = torch.roll(self._slots(d, "encode_diagonals", ns).reshape(ns), g * n1)
        enc = self.encode(z, delta, level=self.L, special=True, log_slots=log_slots)
        baby = [self.galois_elt(b) for b in range(n1)]
        giant = [self.galois_elt(g * n1) for g in range(n2)]
        return baby, giant, [[enc[g, b] for b in range(n1)] for g in range(n2)]

    # ---- wire format ----------------------------------------------
    def serialize(self, x, ntt_form: bool, limb0: int = 0) -> bytes:
        """x [..., nlimbs, N] over limbs [limb0, limb0 + nlimbs) -> an FHEC v1 blob."""
        _check_tensor(x, "x", (self.n,))
        nl = x.shape[-2]
        polys = x.numel() // (nl * self.n)
        lib = load()
        size = lib.fhe_serialized_size(self._ptr, polys, nl)
        buf = ctypes.create_string_buffer(size)
        with torch.cuda.device(self.device):
            check(lib.fhe_serialize(self._ptr, _ptr(x), polys, limb0, nl, int(ntt_form), buf, size,
                                    _stream(x)), "fhe_serialize")
        return buf.raw

    def deserialize(self, blob: bytes):
        """FHEC v1 blob -> (tensor [polys, nlimbs, N] on this context's device, limb0, ntt_form).
        Rejects blobs for another N / other moduli, corrupted or out-of-range data."""
        lib = load()
        polys, limb0, nl, ntt = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int()
        check(lib.fhe_deserialize(self._ptr, blob, len(blob), None, 0, ctypes.byref(polys),
                                  ctypes.byref(limb0), ctypes.byref(nl), ctypes.byref(ntt), None),
              "fhe_deserialize")
        out = _empty(polys.value, nl.value, self.n, dtype=torch.int64, device=self._dev())
        with torch.cuda.device(self.device):
            check(lib.fhe_deserialize(self._ptr, blob, len(blob), _ptr(out), out.numel(), None, None,
                                      None, None, _stream(out)), "fhe_deserialize")
        return out, limb0.value, bool(ntt.value)

    def keyswitch_shard(self, c_all, d2_own, evk_b, evk_a, limb0: int, workspace=None,
                        ranks: int = None):
        """One rank's key-switch given the all-gathered coefficient-form d2.

        c_all: [batch, L, N] (ranks=None), or the rank-major all-gather output
        [ranks, batch, c, N], c = ceil(L / ranks) (fhecore.dist.gather_ranked: no reorder copy);
        d2_own [batch, nlimbs, N] NTT form of limbs [limb0, limb0 + nlimbs); evk_* [dnum,
        nlimbs + K, N].  Returns (ks0, ks1) shaped like d2_own."""
        for t, nm in ((c_all, "c_all"), (d2_own, "d2_own"), (evk_b, "evk_b"), (evk_a, "evk_a")):
            _check_tensor(t, nm, (self.n,))
        nl = d2_own.shape[-2]
        batch = d2_own.numel() // (nl * self.n)
        width = self.L if ranks is None else -(-self.L // ranks)
        if c_all.numel() != (ranks or 1) * batch * width * self.n:
            raise ValueError("keyswitch_shard: c_all must be [batch, L, N] or "
                             "[ranks, batch, ceil(L / ranks), N]")
        if tuple(evk_b.shape) != (self.dnum, nl + self.K, self.n) or evk_a.shape != evk_b.shape:
            raise ValueError("keyswitch_shard: evk slices must be [dnum, nlimbs + K, N]")
        ks0, ks1 = _empty_like(d2_own), _empty_like(d2_own)
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_keyswitch_workspace(self._ptr, nl, batch))
        with torch.cuda.device(self.device):
            if ranks is None:
                check(lib.fhe_keyswitch_shard(self._ptr, _ptr(ks0), _ptr(ks1), _ptr(c_all),
                                              _ptr(d2_own), _ptr(evk_b), _ptr(evk_a), limb0, nl,
                                              batch, _ptr(ws), _stream(d2_own)),
                      "fhe_keyswitch_shard")
            else:
                check(lib.fhe_keyswitch_shard_ranked(self._ptr, _ptr(ks0), _ptr(ks1), _ptr(c_all),
                                                     ranks, _ptr(d2_own), _ptr(evk_b), _ptr(evk_a),
                                                     limb0, nl, batch, _ptr(ws), _stream(d2_own)),
                      "fhe_keyswitch_shard_ranked")
        return ks0, ks1

    def keyswitch_dist(self, comm, d2_own, evk_b, evk_a, chunks: int = 0, workspace=None):
        """Limb-sharded key-switch over an RCCL communicator, all in libfhecore
        (fhe_keyswitch_dist): INTT of this rank's limbs, one ncclAllGather per chunk of the batch
        overlapping the previous chunk's work, then the local key-switch.  comm:
        fhecore.dist.RcclComm; d2_own [batch, nlimbs, N] NTT form of comm.shard(L)'s limbs;
        evk_* [dnum, nlimbs + K, N].  Returns (ks0, ks1) shaped like d2_own."""
        for t, nm in ((d2_own, "d2_own"), (evk_b, "evk_b"), (evk_a, "evk_a")):
            _check_tensor(t, nm, (self.n,))
            if t.device != self._dev():
                raise ValueError(f"keyswitch_dist: {nm} is on {t.device}, the context on "
                                 f"{self._dev()}")
        shard = comm.shard(self.L)
        nl = d2_own.shape[-2]
        if nl != shard.nlimbs:
            raise ValueError(f"keyswitch_dist: d2_own has {nl} limbs, this rank owns "
                             f"{shard.nlimbs}")
        batch = d2_own.numel() // (nl * self.n) if nl else d2_own.shape[0]
        if tuple(evk_b.shape) != (self.dnum, nl + self.K, self.n) or evk_a.shape != evk_b.shape:
            raise ValueError("keyswitch_dist: evk slices must be [dnum, nlimbs + K, N]")
        ks0, ks1 = _empty_like(d2_own), _empty_like(d2_own)
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_keyswitch_dist_workspace(self._ptr, comm.handle, batch, chunks))
        with torch.cuda.device(self.device):
            check(lib.fhe_keyswitch_dist(self._ptr, comm.handle, _ptr(ks0), _ptr(ks1),
                                         _ptr(d2_own), _ptr(evk_b), _ptr(evk_a), batch, chunks,
                                         _ptr(ws), _stream(d2_own)), "fhe_keyswitch_dist")
        return ks0, ks1

    def keyswitch_dist_loopback(self, d2_parts, evk_b_parts, evk_a_parts, chunks: int = 0,
                                workspace=None):
        """fhe_keyswitch_dist's G-rank plan run on this one device (fhe_keyswitch_dist_loopback):
        per-rank lists (rank r: d2 [batch, nlimbs_r, N] NTT form of LimbShard(L, G, r)'s limbs,
        evk slices [dnum, nlimbs_r + K, N]; None for ranks owning no limb).  Returns the per-rank
        (ks0, ks1) lists -- concatenated over the ranks they equal keyswitch()."""
        G = len(d2_parts)
        if not G or len(evk_b_parts) != G or len(evk_a_parts) != G:
            raise ValueError("keyswitch_dist_loopback: one entry per rank in every list")
        from .dist import LimbShard

        batch = None
        ks0, ks1 = [None] * G, [None] * G
        for r in range(G):
            sh = LimbShard(self.L, G, r)
            if sh.nlimbs == 0:
                continue
            d2 = d2_parts[r]
            _check_tensor(d2, f"d2[{r}]", (sh.nlimbs, self.n))
            for t, nm in ((d2, "d2"), (evk_b_parts[r], "evk_b"), (evk_a_parts[r], "evk_a")):
                if nm != "d2":
                    _check_tensor(t, f"{nm}[{r}]", (self.dnum, sh.nlimbs + self.K, self.n))
                # the C side launches on the context's device with these raw pointers
                if t.device != self._dev():
                    raise ValueError(f"keyswitch_dist_loopback: {nm}[{r}] is on {t.device}, "
                                     f"the context on {self._dev()}")
            b = d2.numel() // (sh.nlimbs * self.n)
            if batch is not None and b != batch:
                raise ValueError("keyswitch_dist_loopback: every rank needs the same batch")
            batch = b
            ks0[r], ks1[r] = _empty_like(d2), _empty_like(d2)
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_keyswitch_dist_loopback_workspace(self._ptr, G, batch, chunks))
        arr = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() if t is not None else None  # noqa: E731
                                                  for t in ts])
        ref = next(t for t in d2_parts if t is not None)
        with torch.cuda.device(self.device):
            check(lib.fhe_keyswitch_dist_loopback(self._ptr, G, arr(ks0), arr(ks1), arr(d2_parts),
                                                  arr(evk_b_parts), arr(evk_a_parts), batch,
                                                  chunks, _ptr(ws), _stream(ref)),
                  "fhe_keyswitch_dist_loopback")
        return ks0, ks1


    def keyswitch_dist_hybrid_loopback(self, groups: int, d2_parts, evk_b_parts, evk_a_parts,
                                       chunks: int = 0, workspace=None):
        """The hybrid partition (fhe_dist_hybrid: `groups` ciphertext groups x g limb shards, G =
        len(d2_parts) ranks) run on this one device (fhe_keyswitch_dist_hybrid_loopback).  Rank r
        (group r // g, shard r % g): d2 [group batch, nlimbs, N] NTT form of its group's
        ciphertexts and LimbShard(L, g, r % g)'s limbs (None if it owns none), evk slices
        [dnum, nlimbs + K, N].  Returns the per-rank (ks0, ks1) lists."""
        G = len(d2_parts)
        if not G or groups < 1 or G % groups or len(evk_b_parts) != G or len(evk_a_parts) != G:
            raise ValueError("keyswitch_dist_hybrid_loopback: one entry per rank, groups | ranks")
        from .dist import LimbShard

        g = G // groups
        ks0, ks1 = [None] * G, [None] * G
        job = 0
        for r in range(G):
            sh = LimbShard(self.L, g, r % g)
            d2 = d2_parts[r]
            if sh.nlimbs == 0 or d2 is None:
                continue
            _check_tensor(d2, f"d2[{r}]", (sh.nlimbs, self.n))
            for t, nm in ((evk_b_parts[r], "evk_b"), (evk_a_parts[r], "evk_a")):
                _check_tensor(t, f"{nm}[{r}]", (self.dnum, sh.nlimbs + self.K, self.n))
            for t, nm in ((d2, "d2"), (evk_b_parts[r], "evk_b"), (evk_a_parts[r], "evk_a")):
                if t.device != self._dev():
                    raise ValueError(f"keyswitch_dist_hybrid_loopback: {nm}[{r}] is on "
                                     f"{t.device}, the context on {self._dev()}")
            if r % g == 0:
                job += d2.numel() // (sh.nlimbs * self.n)
            ks0[r], ks1[r] = _empty_like(d2), _empty_like(d2)
        lib = load()
        ws = workspace if workspace is not None else self.workspace(
            lib.fhe_keyswitch_dist_hybrid_loopback_workspace(self._ptr, G, groups, job, chunks))
        arr = lambda ts: (ctypes.c_void_p * G)(*[t.data_ptr() if t is not None else None  # noqa: E731
                                                  for t in ts])
        ref = next(t for t in d2_parts if t is not None)
        with torch.cuda.device(self.device):
            check(lib.fhe_keyswitch_dist_hybrid_loopback(
                self._ptr, G, groups, arr(ks0), arr(ks1), arr(d2_parts), arr(evk_b_parts),
                arr(evk_a_parts), job, chunks, _ptr(ws), _stream(ref)),
                "fhe_keyswitch_dist_hybrid_loopback")
        return ks0, ks1


class Graph:
    """Capture libfhecore calls issued on the current stream into a HIP graph and replay them
    (fhe_graph_*).  The tensors a captured call reads and writes are baked into the graph:
    outputs and workspaces that the Context methods allocate inside the block are kept alive by
    the Graph (``Graph.tensors``; read results from there or pass ``out=``), and caller-owned
    tensors must outlive it.  Every call is given a workspace -- the one passed in, or one this
    module allocates and the Graph keeps -- since the context's internal one is refused while
    capturing (include/fhecore.h)::

        with fhecore.Graph() as g:
            ctx.mul_relin(a, b, kb, ka, workspace=ws, out=out)
        g.launch()
    """

    def __init__(self):
        self._g = None
        self.tensors = []

    def __enter__(self):
        self._stream = torch.cuda.current_stream()
        check(load().fhe_graph_begin(ctypes.c_void_p(self._stream.cuda_stream)), "fhe_graph_begin")
        _CAPTURE.keep = self.tensors
        return self

    def __exit__(self, exc_type, exc, tb):
        _CAPTURE.keep = None
        g = ctypes.c_void_p()
        rc = load().fhe_graph_end(ctypes.c_void_p(self._stream.cuda_stream), ctypes.byref(g))
        if exc_type is None:
            check(rc, "fhe_graph_end")
            self._g = g
        return False

    def launch(self):
        check(load().fhe_graph_launch(self._g, ctypes.c_void_p(self._stream.cuda_stream)),
              "fhe_graph_launch")

    def __del__(self):
        if getattr(self, "_g", None):
            try:
                load().fhe_graph_destroy(self._g)
            except Exception:  # interpreter shutdown
                pass
