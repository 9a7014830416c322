"""Polar-code helpers for the SC-list tests: the ctypes binding to the C restatement of the
vendored SC-list decoder (oracle/build/libpolar_oracle.so -- the CHECKER only), a code
specification builder in the reference's spec format (out/external/MixedKernelEncoder.cpp:
7-98), and an AWGN channel producing the decoder's LLRs.

Only tests/ import this.
"""
import ctypes as C
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "oracle", "build", "libpolar_oracle.so")

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-s", "-C", os.path.join(REPO, "oracle"), "oracle"], check=True)
        L = C.CDLL(LIB)
        vp = C.c_void_p
        L.plr_create.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]
        L.plr_create.restype = vp
        L.plr_destroy.argtypes = [vp]
        L.plr_dims.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.plr_encode.argtypes = [vp, vp, vp]
        L.plr_encode_unshortened.argtypes = [vp, vp, vp]
        L.plr_extract_info.argtypes = [vp, vp, vp]
        L.plr_decode.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class PolarOracle:
    """One code from its specification text; SC-list decode with list size L."""

    def __init__(self, spec, kernel_dir=None):
        msg = C.create_string_buffer(512)
        self.h = lib().plr_create(spec.encode(), (kernel_dir or "").encode(), msg, 512)
        if not self.h:
            raise ValueError(msg.value.decode())
        n, k, u = C.c_int(), C.c_int(), C.c_int()
        lib().plr_dims(self.h, C.byref(n), C.byref(k), C.byref(u))
        self.N, self.K, self.U = n.value, k.value, u.value

    def __del__(self):
        if getattr(self, "h", None):
            lib().plr_destroy(self.h)
            self.h = None

    def encode(self, info):
        info = np.ascontiguousarray(info, np.uint8)
        out = np.zeros((info.shape[0], self.N), np.uint8)
        for b in range(info.shape[0]):
            lib().plr_encode(self.h, _p(info[b]), _p(out[b]))
        return out

    def encode_unshortened(self, info):
        info = np.ascontiguousarray(info, np.uint8)
        out = np.zeros(self.U, np.uint8)
        lib().plr_encode_unshortened(self.h, _p(info), _p(out))
        return out

    def extract_info(self, ucw):
        ucw = np.ascontiguousarray(ucw, np.uint8)
        out = np.zeros(self.K, np.uint8)
        lib().plr_extract_info(self.h, _p(ucw), _p(out))
        return out

    def decode(self, llr, L):
        """llr [N] float32 -> (count, info [L][K], codewords [L][N], metrics [L])."""
        llr = np.ascontiguousarray(llr, np.float32)
        info = np.zeros((L, self.K), np.uint8)
        cw = np.zeros((L, self.N), np.uint8)
        met = np.zeros(L, np.float32)
        n = lib().plr_decode(self.h, L, _p(llr), _p(info), _p(cw), _p(met))
        assert n >= 1
        return n, info, cw, met

    def decode_batch(self, llrs, L, threads=None):
        """Rows decoded independently, over host threads (plr_decode keeps no global state;
        ctypes releases the GIL during the call)."""
        from concurrent.futures import ThreadPoolExecutor

        from oracle_lib import host_threads
        B = llrs.shape[0]
        cnt = np.zeros(B, np.int32)
        info = np.zeros((B, L, self.K), np.uint8)
        cw = np.zeros((B, L, self.N), np.uint8)
        met = np.zeros((B, L), np.float32)

        def one(b):
            cnt[b], info[b], cw[b], met[b] = self.decode(llrs[b], L)

        with ThreadPoolExecutor(max_workers=min(threads or host_threads(), max(1, B))) as ex:
            list(ex.map(one, range(B)))
        return cnt, info, cw, met


def pw_order(n):
    """Polarization-weight reliability of the 2^n bit channels (index bits weighted by
    2^(b/4)); least reliable first. A standard construction, used here only to pick
    frozen sets for test and benchmark codes."""
    U = 1 << n
    w = [sum(((i >> b) & 1) * 2.0 ** (b / 4.0) for b in range(n)) for i in range(U)]
    return sorted(range(U), key=lambda i: (w[i], i))


def arikan_spec(n, K, dyn=0, punct=(), seed=0, short=(), freeze=()):
    """Spec text of a length-2^n Arikan polar code of dimension K: the U - K least reliable
    symbols frozen (`dyn` of them dynamically, each as the XOR of two earlier symbols),
    `punct` punctured and `short` shortened positions (N = U - len(punct) - len(short)).
    `freeze` are frozen to 0 whatever their rank, within the U - K (what makes a symbol always 0,
    so that it can be shortened: see shorten())."""
    U = 1 << n
    rng = np.random.default_rng(seed)
    frozen = sorted(list(freeze) + [i for i in pw_order(n) if i not in freeze][:U - K - len(freeze)])
    dynset = set(rng.choice([f for f in frozen if f >= 2 and f not in freeze], size=min(dyn, len(frozen)),
                            replace=False).tolist()) if dyn else set()
    lines = [f"{U - len(punct) - len(short)} {K} 0 {n} {len(short)} {len(punct)}", " ".join(["A"] * n)]
    if short or punct:
        lines.append(" ".join(str(p) for p in tuple(short) + tuple(punct)))
    for f in frozen:
        if f in dynset:
            a, b = sorted(rng.choice(f, size=2, replace=False).tolist())
            lines.append(f"3 {a} {b} {f}")
        else:
            lines.append(f"1 {f}")
    return "\n".join(lines) + "\n"


DENSE_WIDTHS = (1, 2, 3, 2, 5)  # terms before the frozen symbol: a plain copy, the usual two, more


def dense_constraints(U, K, active, pivot, widths, seed, rank, lo_info, late=0):
    """The U - K constraint lines of a code whose dynamic freezing is DENSE: `active` constraints
    all live across symbol `pivot` -- each has an information symbol below pivot as its first term
    and freezes a symbol at or above pivot, its other terms are information symbols in between --
    and `late` more that start past the pivot, after others have retired, so that they take reused
    mask bits. The frozen set is whatever makes this possible, no good code: the lo_info symbols
    below pivot and the K - lo_info at or above it that come last in `rank` carry information,
    `active + late` of the others at or above pivot (drawn by seed) are dynamically frozen, the
    rest statically.

    widths: terms BEFORE the frozen symbol (the line holds one number more) of as many constraints,
    the widest on the last frozen symbols, where the most information symbols lie below; the others
    cycle through DENSE_WIDTHS. The last information symbol below pivot is the hub: a term of every
    constraint that can hold it, one in five left out, so its correction word has bits of both
    halves of the mask set without being all ones."""
    rng = np.random.default_rng(seed)
    place = {s: r for r, s in enumerate(rank)}
    lo = sorted(range(pivot), key=place.get, reverse=True)
    hi = sorted(range(pivot, U), key=place.get, reverse=True)
    assert 2 <= lo_info <= len(lo) and 0 <= K - lo_info <= len(hi) - active - late, (lo_info, K, len(hi))
    info_lo = sorted(lo[:lo_info])
    info = sorted(info_lo + hi[:K - lo_info])
    dyn = sorted(rng.choice(hi[K - lo_info:], size=active + late, replace=False).tolist())
    early, tail = dyn[:active], dyn[active:]
    hub = info_lo[-1]
    first = rng.choice(info_lo, size=active).tolist()
    want = [DENSE_WIDTHS[i % len(DENSE_WIDTHS)] for i in range(active)]
    plain = active - len(widths)
    assert plain >= 3
    first[0], first[plain - 1], first[plain - 2] = info_lo[0], hub, hub  # the hub's own constraints take the last bits
    for i, w in enumerate(sorted(widths)):  # the widest last
        want[plain + i], first[plain + i] = w, info_lo[0]
    cons = {}
    for p, (a, f) in enumerate(sorted(zip(first, early))):  # p: the order the mask bits are handed out in
        w = want[early.index(f)]
        between = [s for s in info if a < s < f and s != hub]
        terms = [a] + ([hub] if hub > a and w >= 2 and p % 5 != 1 else [])
        short = len(between) < w - len(terms)  # only a width of the cycle may shrink to what lies between
        assert not (short and early.index(f) >= plain), f"constraint on {f}: {w} terms asked, {len(between) + len(terms)} symbols"
        terms += rng.choice(between, size=len(between) if short else w - len(terms), replace=False).tolist()
        cons[f] = sorted(terms) + [f]
    for k, f in enumerate(tail):  # after k + 1 of the early ones have retired, as late as possible
        a = max((s for s in info if early[k] < s < f), default=None)
        assert a is not None, f"no information symbol between {early[k]} and {f} (another seed)"
        cons[f] = [a, f]
    return [" ".join(str(v) for v in [len(cons[f])] + cons[f]) if f in cons else f"1 {f}"
            for f in range(U) if f not in info]


def dense_arikan_spec(n, K, active, pivot, widths=(), seed=0, lo_info=None, late=0):
    """arikan_spec's twin for dense dynamic freezing (dense_constraints): rank is pw_order, and
    lo_info defaults to half of K. Nothing shortened or punctured."""
    U = 1 << n
    lines = dense_constraints(U, K, active, pivot, widths, seed, pw_order(n), K // 2 if lo_info is None else lo_info, late)
    return "\n".join([f"{U} {K} 0 {n} 0 0", " ".join(["A"] * n)] + lines) + "\n"


# ---- what a specification's dynamic freezing amounts to, from its text alone (nothing below
# calls the product or the oracle)

def spec_constraints(spec):
    """The freezing constraints in file order, each the list of its terms with the frozen symbol
    last (a static one: the symbol alone)."""
    tok = spec.split()
    N, K, _, layers, nsh, npu = (int(v) for v in tok[:6])
    pos, cons = 6 + layers + nsh + npu, []
    while pos < len(tok):
        w = int(tok[pos])
        cons.append([int(v) for v in tok[pos + 1:pos + 1 + w]])
        pos += 1 + w
    assert len(cons) == N + nsh + npu - K
    return cons


def max_active(spec):
    """The most dynamic constraints live at once. One is live from its first term up to, not
    including, its frozen symbol: at a symbol the constraint frozen there retires before those
    that start there begin."""
    dyn = [(c[0], c[-1]) for c in spec_constraints(spec) if len(c) > 1]
    return max((sum(a <= i < f for a, f in dyn) for i in sorted({a for a, _ in dyn})), default=0)


def constraint_bits(spec):
    """{frozen symbol: mask bit} by the lowest-free-bit rule replayed over the symbols in order: at
    symbol i the bit of the constraint frozen at i is freed, then every constraint whose first term
    is i takes the lowest free bit, in the order of their frozen symbols. ValueError where none of
    the 64 is free."""
    dyn = sorted((c[0], c[-1]) for c in spec_constraints(spec) if len(c) > 1)
    free, bits = set(range(64)), {}
    for i in sorted({a for a, _ in dyn} | {f for _, f in dyn}):
        if i in bits:
            free.add(bits[i])
        for a, f in dyn:
            if a == i:
                if not free:
                    raise ValueError("more than 64 constraints live at once")
                bits[f] = min(free)
                free.remove(bits[f])
    return bits


def correction_words(spec):
    """{symbol: 64-bit word}: the mask bits that change when the symbol is 1 (each term sets its
    constraint's bit; the frozen symbol clears it for reuse)."""
    bits, corr = constraint_bits(spec), {}
    for c in spec_constraints(spec):
        if len(c) > 1:
            for s in c:
                corr[s] = corr.get(s, 0) ^ (1 << bits[c[-1]])
    return corr


def spec_inputs(spec, U, info):
    """The encoder inputs u [B][U] of the information words info [B][K]: information bits at the
    unfrozen symbols in order, each frozen symbol the XOR of its constraint's listed terms."""
    info = np.asarray(info, np.uint8)
    by_symbol = {c[-1]: c[:-1] for c in spec_constraints(spec)}
    u, k = np.zeros((len(info), U), np.uint8), 0
    for i in range(U):
        if i in by_symbol:
            for t in by_symbol[i]:
                u[:, i] ^= u[:, t]
        else:
            u[:, i] = info[:, k] & 1
            k += 1
    assert k == info.shape[1]
    return u


def kernel_transform(u, kernels):
    """u [B][U] through the layers' kernels (l x l 0/1 matrices, outermost first), innermost
    layer first: (y_i, y_{i+d}, ..) = (x_i, x_{i+d}, ..) M in every block of l d symbols."""
    x, B, stride = np.asarray(u, np.int64), len(u), 1
    for M in reversed(kernels):
        l = len(M)
        x = (np.einsum("ji,bkjs->bkis", np.asarray(M, np.int64), x.reshape(B, -1, l, stride)) & 1).reshape(B, -1)
        stride *= l
    return x.astype(np.uint8)


ARIKAN = np.array([[1, 0], [1, 1]], np.uint8)


def always_zero_symbols(spec, kernel_dir=None):
    """The symbols of the unshortened codeword that are 0 for every information word: 0 in the
    encoding of the zero word and of the K unit words (the code is affine in the information
    bits). `spec` shortens and punctures nothing."""
    o = PolarOracle(spec, kernel_dir)
    assert o.N == o.U
    seen = o.encode_unshortened(np.zeros(o.K, np.uint8))
    for k in range(o.K):
        seen |= o.encode_unshortened(np.eye(o.K, dtype=np.uint8)[k])
    return [int(i) for i in np.flatnonzero(seen == 0)]


def shorten(build, U, s, punct=(), kernel_dir=None, zero_form=None):
    """A valid shortened specification from a builder build(short=, freeze=, punct=) such as
    arikan_spec: the last s encoder inputs are frozen to 0, and s of the symbols that this makes
    always 0 are shortened -- the lowest-numbered ones, so not the run at the very end where the
    kernels leave a choice. zero_form(spec) rewrites the unshortened specification for
    always_zero_symbols (named kernels in their matrix form, which the oracle takes)."""
    freeze = tuple(range(U - s, U))
    plain = build(short=(), freeze=freeze, punct=())
    zeros = [z for z in always_zero_symbols(zero_form(plain) if zero_form else plain, kernel_dir) if z not in punct]
    assert len(zeros) >= s, (zeros, s)
    return build(short=tuple(zeros[:s]), freeze=freeze, punct=tuple(punct))


def awgn_llr(cw, snr_db, rate, seed):
    """BPSK with bit 1 -> +1 (headers/external/Modem.h:64) over AWGN at Eb/N0 snr_db, LLR
    -2y/sigma^2 (Modem.h:78): positive favours 0, as the decoder reads it."""
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(1.0 / (2.0 * rate * 10.0 ** (snr_db / 10.0)))
    x = np.where(cw != 0, 1.0, -1.0)
    y = x + sigma * rng.standard_normal(cw.shape)
    return (-2.0 * y / sigma ** 2).astype(np.float32)
