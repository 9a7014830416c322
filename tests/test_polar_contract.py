"""The polar decoders' contract where the rest of the suite does not look: shortened codes (the
100000 of LoadLLRs, plist::chan_llr) through every list kernel, the genie and the device
pipeline; lists shorter than L (2^K < L) with every output row past the count, and guard bytes
around the device buffers, left as they were; cw = NULL; the epilogue's packed and byte stores at
every (K mod 4, N mod 4) with K past a record word and a lane round; K = 0 and K = U; the genie
entry points on tiered contexts.

Everything is bit for bit. Expected lists come from the C oracle (oracle/polar_oracle.c, pinned to
the compiled vendored library by tests/test_polar_reference.py -- with this module's three
shortened fixtures, polar_ref_short_*, among the ones it globs), the LLR stream from
tests/philox_lib.py, the counters from tests/test_polar_sim.py's numpy table. Two exceptions, both
where the claim IS the equality of two call forms: cw = NULL against the call with a cw buffer, and
the genie on a tiered context against an LDS-state one.

The oracle restates neither G nor A5, so the named code A5 x G x A has no CPU reference for its
lists (and none exists with a list: the reference's G state does not survive a clone outside the
innermost layer). For it the LDS state is checked for what needs no decoder -- the
count 2^K, every information word once, each codeword row the matrix-form encoding of its
information row, metrics in the final order, and the sentinel -- and the tiered state against the
LDS one, as tests/test_polar_mixed_tiered.py does. At L = 1 the reference is defined: there the
shortened code's lists are the recorded ones of named_ref_A5_G_A_short (large LLRs included).

K = 0 is a code the library takes (parse_spec accepts it, the record layout and the buffers are
sized for max(K, 1)): decode returns the one frozen word with its metric; only generate_device,
which needs a rate, refuses it.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import named_lib as NL
import philox_lib as P
from bchk_pkg import load
from genie_lib import GenieCode, column_sums
import short_codes
from polar_lib import PolarOracle, arikan_spec, awgn_llr
from short_codes import SHORT, matrix_form
from test_polar_mixed import mixed_spec

SENT = 0xA5
SENT32 = np.uint32(0xA5A5A5A5)
SENT_COUNT = -12345
B_WORDS = 32


# ---------------------------------------------------------------- kernel files, specifications

_KDIR = []


@pytest.fixture(scope="module", autouse=True)
def kdir(tmp_path_factory):
    """The kernel files (short_codes.write_kernels), for every test of the module."""
    _KDIR.append(short_codes.write_kernels(tmp_path_factory.mktemp("contract_kernels")))
    yield _KDIR[0]
    _KDIR.clear()


def kernel_dir():
    return _KDIR[0]


ARIKAN_SHORT = ["arikan_n6", "arikan_n7"]
MIXED_SHORT = ["bch8_A_A", "bch16_A", "A_bch16", "A_bch32f", "k3_k4_A"]


def short_spec(name):
    return short_codes.short_spec(name, kernel_dir())


def header(spec):
    N, K, _, nl, nsh, npu = (int(t) for t in spec.split()[:6])
    return N, K, nl, nsh, npu


def dropped(spec):
    """(shortened, punctured) symbol lists of the specification."""
    N, K, nl, nsh, npu = header(spec)
    tok = [int(t) for t in spec.split()[6 + nl:6 + nl + nsh + npu]]
    return tok[:nsh], tok[nsh:]


def oracle(spec):
    return PolarOracle(matrix_form(spec), kernel_dir())


# ---------------------------------------------------------------- the comparer

def sentinel_outputs(B, L, K, N):
    """(count, info, cw, metric) host arrays holding the sentinel."""
    return (np.full(B, SENT_COUNT, np.int32), np.full((B, L, K), SENT, np.uint8), np.full((B, L, N), SENT, np.uint8),
            np.full((B, L), SENT32, np.uint32).view(np.float32))


def assert_strict(got, want, what="", cw=True):
    """got: outputs that held the sentinel before the call; want: (count, info, cw, metric) with
    rows [:count] valid (PolarOracle.decode_batch). Rows [:count] equal bit for bit, in list
    order; rows [count:L] still hold the sentinel. cw=False: the cw buffer was not passed, and
    holds the sentinel everywhere."""
    gc, gi, gw, gm = got
    wc, wi, ww, wm = want
    np.testing.assert_array_equal(gc, wc, err_msg=f"{what}: counts")
    gm, wm = np.ascontiguousarray(gm).view(np.uint32), np.ascontiguousarray(wm).view(np.uint32)
    for b in range(len(wc)):
        c = int(wc[b])
        np.testing.assert_array_equal(gi[b, :c], wi[b, :c], err_msg=f"{what}: info, word {b}")
        np.testing.assert_array_equal(gm[b, :c], wm[b, :c], err_msg=f"{what}: metric bits, word {b}")
        if cw:
            np.testing.assert_array_equal(gw[b, :c], ww[b, :c], err_msg=f"{what}: codewords, word {b}")
        else:
            c = 0
        assert (gw[b, c:] == SENT).all(), f"{what}: codeword rows past the count written, word {b}"
        c = int(wc[b])
        assert (gi[b, c:] == SENT).all(), f"{what}: info rows past the count written, word {b}"
        assert (gm[b, c:] == SENT32).all(), f"{what}: metric rows past the count written, word {b}"


def decode_host(d, llr, cw=True):
    """bchk_polar_decode_host on sentinel-filled outputs (cw=False: cw = NULL, the array returned
    is one the library never saw)."""
    llr = np.ascontiguousarray(llr, np.float32)
    cnt, info, cwa, met = sentinel_outputs(len(llr), d.L, d.K, d.N)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = load().lib().bchk_polar_decode_host(d.handle, p(llr), len(llr), p(info), p(cwa) if cw else None, p(met), p(cnt))
    assert rc == 0, load().lib().bchk_last_error().decode()
    return cnt, info, cwa, met


GUARD = 256


class Guarded:
    """A device buffer of `nbytes` inside a larger 0xA5-filled byte tensor: it starts at a multiple
    of 256 bytes, with at least 256 guard bytes on each side."""

    def __init__(self, nbytes):
        import torch
        self.n = nbytes
        body = (max(nbytes, 1) + GUARD - 1) // GUARD * GUARD
        self.t = torch.full((2 * GUARD + body + GUARD,), SENT, dtype=torch.uint8, device="cuda:0")
        self.off = GUARD + (-self.t.data_ptr()) % GUARD
        self.ptr = self.t.data_ptr() + self.off
        assert self.ptr % GUARD == 0 and self.off >= GUARD and len(self.t) - self.off - nbytes >= GUARD

    def read(self, dtype, shape, what):
        h = self.t.cpu().numpy()
        assert (h[:self.off] == SENT).all(), f"{what}: bytes before the buffer written"
        assert (h[self.off + self.n:] == SENT).all(), f"{what}: bytes after the buffer written"
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)


def decode_device(d, llr, cw=True):
    """bchk_polar_decode_device into guarded, sentinel-filled device buffers; the guards are
    checked here, the rows by the caller (assert_strict)."""
    import torch
    llr = np.ascontiguousarray(llr, np.float32)
    B = len(llr)
    t_llr = torch.from_numpy(llr).to("cuda:0")
    g_info, g_cw = Guarded(B * d.L * d.K), Guarded(B * d.L * d.N)
    g_met, g_cnt = Guarded(4 * B * d.L), Guarded(4 * B)
    torch.cuda.synchronize()
    d.decode_device(t_llr.data_ptr(), B, g_info.ptr, g_cw.ptr if cw else None, g_met.ptr, g_cnt.ptr)
    d.sync()
    cnt = g_cnt.read(np.int32, (B,), "count")
    assert ((cnt >= 1) & (cnt <= d.L)).all(), cnt
    return (cnt, g_info.read(np.uint8, (B, d.L, d.K), "info"), g_cw.read(np.uint8, (B, d.L, d.N), "cw"),
            g_met.read(np.float32, (B, d.L), "metric"))


# ---------------------------------------------------------------- contexts and workloads

def n_layers(spec):
    return header(spec)[2]


def all_arikan(spec):
    return all(n in ("A", "a") for n in spec.split("\n")[1].split())


def states(spec, kinds=("lds", "tiered", "tiered_mixed")):
    """(label, state, split) of every way a context keeps this code's state, at every split."""
    out = []
    if "lds" in kinds:
        out.append(("lds", "lds", None))
    if "tiered" in kinds and all_arikan(spec):
        out += [(f"tiered-{s}", "tiered", s) for s in range(1, n_layers(spec) + 1)]
    if "tiered_mixed" in kinds:
        out += [(f"tiered_mixed-{s}", "tiered_mixed", s) for s in range(1, n_layers(spec) + 1)]
    return out


class context:
    def __init__(self, spec, L, state="lds", split=None):
        self.d = load().PolarListDecoder(spec, L, kernel_dir=kernel_dir(), state=state, split=split)

    def __enter__(self):
        return self.d

    def __exit__(self, *a):
        self.d.close()


def batches(spec, B=B_WORDS, seed=0):
    """LLR batches of one code: Eb/N0 0 and 3 dB; the first quantised, so that ties meet the
    shortened symbols' 100000; and the second times short_codes.LARGE, beside which the f32 sums
    round as the oracle's do, and without which no list depends on the mapped value."""
    o = oracle(spec)
    rng = np.random.default_rng(1000 + seed)
    rate = o.K / o.N if o.K else 0.5
    out = []
    for snr in (0.0, 3.0):
        info = rng.integers(0, 2, (B, o.K)).astype(np.uint8)
        out.append(awgn_llr(o.encode(info), snr, rate, seed=seed + int(snr)))
    out.append(np.round(out[0] / 4.0).astype(np.float32))
    out.append(out[1] * short_codes.LARGE)
    assert 1000.0 < np.abs(out[3]).max() < 100000.0
    return out


_want = {}


def expected(key, spec, L, B=B_WORDS):
    """The oracle's lists of the code's batches at list size L: computed once, shared, unchanged."""
    if (key, L, B) not in _want:
        o = oracle(spec)
        llrs = batches(spec, B, seed=len(key))
        _want[(key, L, B)] = (llrs, [o.decode_batch(llr, L) for llr in llrs])
    return _want[(key, L, B)]


def check_against_oracle(key, spec, L, state, split, label):
    llrs, wants = expected(key, spec, L)
    with context(spec, L, state, split) as d:
        assert d.split == (split or 0)
        for i, (llr, want) in enumerate(zip(llrs, wants)):
            assert_strict(decode_host(d, llr), want, f"{key} {label} L={L} batch {i}")


# ================================================================ CPU

def _old_arikan_spec(n, K, dyn=0, punct=(), seed=0):
    U = 1 << n
    rng = np.random.default_rng(seed)
    from polar_lib import pw_order
    frozen = sorted(pw_order(n)[:U - K])
    dynset = set(rng.choice([f for f in frozen if f >= 2], size=min(dyn, len(frozen)), replace=False).tolist()) if dyn else set()
    lines = [f"{U - len(punct)} {K} 0 {n} 0 {len(punct)}", " ".join(["A"] * n)]
    if punct:
        lines.append(" ".join(str(p) for p in punct))
    for f in frozen:
        if f in dynset:
            a, b = sorted(rng.choice(f, size=2, replace=False).tolist())
            lines.append(f"3 {a} {b} {f}")
        else:
            lines.append(f"1 {f}")
    return "\n".join(lines) + "\n"


def test_spec_builders_write_what_they_wrote_without_short():
    """short=() / freeze=() leave the text as the builders wrote it before they had them: the
    earlier arikan_spec restated above, and for mixed_spec the recorded fixtures' '@spec'."""
    from test_polar_sclist import CODES
    for n, K, dyn, punct in CODES + [(6, 30, 5, ()), (14, 8192, 40, (3, 9000))]:
        for seed in (0, n, 7 * n + 4):
            assert arikan_spec(n, K, dyn=dyn, punct=punct, seed=seed) == _old_arikan_spec(n, K, dyn, punct, seed)
    import importlib.util
    import polar_ref_lib as R
    mg = importlib.util.spec_from_file_location("make_golden", os.path.join(R.REPO, "oracle", "make_golden.py"))
    gen = importlib.util.module_from_spec(mg)
    mg.loader.exec_module(gen)
    for layers, K, dyn, punct in gen.POLAR_MIXED:
        fx = R.load_fixture(os.path.join(R.GOLD, "polar_ref_mixed_" + "_".join(layers) + ".txt.gz"))
        assert mixed_spec(layers, K, dyn, punct, seed=len(layers) * 11 + K) == fx.spec


@pytest.mark.parametrize("name", list(SHORT))
def test_shortened_symbols_are_always_zero(name, kdir):
    """The precondition of every shortened code used here: its shortened symbols are 0 in the
    unshortened encoding of 32 random information words (and the transmitted symbols are the rest)."""
    spec = short_spec(name)
    o = oracle(spec)
    sh, pu = dropped(spec)
    N, K, nl, nsh, npu = header(spec)
    assert nsh == len(sh) > 0 and o.U == N + nsh + npu and not set(sh) & set(pu)
    info = np.random.default_rng(len(name)).integers(0, 2, (32, K)).astype(np.uint8)
    keep = [i for i in range(o.U) if i not in sh and i not in pu]
    for w, cw in zip(info, o.encode(info)):
        u = o.encode_unshortened(w)
        assert not u[sh].any(), (name, sh)
        np.testing.assert_array_equal(u[keep], cw)
    print(name, "U", o.U, "K", K, "shortened", sh, "punctured", pu)


def test_the_mixed_specification_shortens_punctures_and_freezes_dynamically():
    spec = short_spec("arikan_n7")
    assert header(spec) == (123, 60, 7, 3, 2) and spec.count("\n3 ") == 4
    assert header(short_spec("arikan_n6")) == (59, 24, 6, 5, 0) and dropped(short_spec("arikan_n6"))[0] == [59, 60, 61, 62, 63]


# codes whose lists are shorter than L: name -> (specification, L, count)
def _a5ga(K):
    return NL.named_spec(("A5", "G", "A"), K, seed=3)


SHORT_LISTS = {
    "A3-K1-L32": (lambda: arikan_spec(3, 1), 32, 2),
    "A5-K2-L8": (lambda: arikan_spec(5, 2), 8, 4),
    "A5-K3-L32": (lambda: arikan_spec(5, 3), 32, 8),
    "k4_A-K2-L16": (lambda: mixed_spec(("k4", "A"), 2, seed=2), 16, 4),
    "A5_G_A-K2-L8": (lambda: _a5ga(2), 8, 4),
}
EDGE_K = {"A4-K0-L4": (lambda: arikan_spec(4, 0), 4, 1), "A4-K16-L8": (lambda: arikan_spec(4, 16), 8, 8)}


@pytest.mark.parametrize("name", [n for n in list(SHORT_LISTS) + list(EDGE_K) if "G" not in n])
def test_oracle_list_lengths(name, kdir):
    """The oracle on the short-list, K = 0 and K = U codes: count min(2^K, L); with 2^K <= L every
    information word exactly once, best metric first; the K = 0 row is the frozen word."""
    build, L, count = dict(SHORT_LISTS, **EDGE_K)[name]
    spec = build()
    o = oracle(spec)
    assert count == min(1 << o.K, L)
    llr = batches(spec, 8)[0]
    cnt, info, cw, met = o.decode_batch(llr, L)
    assert (cnt == count).all()
    for b in range(len(llr)):
        if (1 << o.K) <= L:
            assert len({r.tobytes() for r in info[b, :count]}) == 1 << o.K
        np.testing.assert_array_equal(cw[b, :count], o.encode(info[b, :count]))
        assert (np.diff(met[b, :count]) <= 0).all()


# ================================================================ A. shortened codes

@pytest.mark.gpu
@pytest.mark.parametrize("name", ARIKAN_SHORT)
@pytest.mark.parametrize("L", [1, 4, 32])
def test_gpu_shortened_arikan_lds(name, L, kdir):
    check_against_oracle(name, short_spec(name), L, "lds", None, "lds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARIKAN_SHORT)
@pytest.mark.parametrize("L", [2, 8])
def test_gpu_shortened_arikan_tiered_every_split(name, L, kdir):
    """The shortened symbols' 100000 arrives through the workspace copy of the channel LLRs."""
    spec = short_spec(name)
    for label, state, split in states(spec, ("tiered",)):
        check_against_oracle(name, spec, L, state, split, label)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MIXED_SHORT)
@pytest.mark.parametrize("L", [1, 8])
def test_gpu_shortened_mixed_lds(name, L, kdir):
    check_against_oracle(name, short_spec(name), L, "lds", None, "lds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", MIXED_SHORT)
def test_gpu_shortened_mixed_tiered_every_split(name, kdir):
    spec = short_spec(name)
    for label, state, split in states(spec, ("tiered_mixed",)):
        check_against_oracle(name, spec, 4, state, split, label)


def named_contract(spec, got, what):
    """What holds of a named code's lists without a decoder to compare with: every row [:count] a
    codeword -- the matrix-form encoding of its information row -- no word twice, metrics in the
    final order (descending), the sentinel past the count."""
    o = oracle(spec)
    cnt, info, cw, met = got
    for b in range(len(cnt)):
        c = int(cnt[b])
        np.testing.assert_array_equal(cw[b, :c], o.encode(info[b, :c]), err_msg=f"{what}: word {b}")
        assert len({r.tobytes() for r in info[b, :c]}) == c, f"{what}: a word twice, word {b}"
        assert (np.diff(met[b, :c]) <= 0).all(), f"{what}: list order, word {b}"
    assert_strict(got, got, what)  # the rows past each count


@pytest.mark.gpu
def test_gpu_shortened_named_code_in_both_mixed_states(kdir):
    """A5 x G x A with one shortened symbol. Noiseless words decode to themselves at metric 0 in
    the LDS state (a mapped value that contradicted the shortened symbol's 0 would cost its
    magnitude); noisy ones keep the named contract there, and the tiered state at every split gives
    the LDS state's lists bit for bit."""
    spec = short_spec("A5_G_A")
    o = oracle(spec)
    info = np.random.default_rng(5).integers(0, 2, (B_WORDS, o.K)).astype(np.uint8)
    clean = np.where(o.encode(info) != 0, -6.0, 6.0).astype(np.float32)
    for L in (1, 8):
        with context(spec, L) as d:
            cnt, inf, cw, met = decode_host(d, clean)
            np.testing.assert_array_equal(inf[:, 0], info)
            assert (met[:, 0] == 0.0).all()
            named_contract(spec, (cnt, inf, cw, met), f"A5_G_A lds L={L} noiseless")
            lists = [decode_host(d, llr) for llr in batches(spec, seed=6)]
        for i, got in enumerate(lists):
            named_contract(spec, got, f"A5_G_A lds L={L} batch {i}")
    llrs = batches(spec, seed=6)
    with context(spec, 4) as d:
        wants = [decode_host(d, llr) for llr in llrs]
    for label, state, split in states(spec, ("tiered_mixed",)):
        with context(spec, 4, state, split) as d:
            for i, (llr, want) in enumerate(zip(llrs, wants)):
                assert_strict(decode_host(d, llr), want, f"A5_G_A {label} batch {i}")


def recorded_lists(fx, L):
    """Fixture.decoded(L) in the comparer's form."""
    rows = fx.decoded(L)
    N, K = header(fx.spec)[:2]
    cnt = np.array([r[0] for r in rows], np.int32)
    info, cw, met = np.zeros((len(rows), L, K), np.uint8), np.zeros((len(rows), L, N), np.uint8), np.zeros((len(rows), L), np.uint32)
    for b, (c, wi, ww, wm) in enumerate(rows):
        info[b, :c], cw[b, :c], met[b, :c] = wi, ww, wm
    return cnt, info, cw, met.view(np.float32)


def test_named_short_fixture_is_what_it_is_for():
    fx = NL.fixture(os.path.join(NL.R.GOLD, f"named_ref_{short_codes.NAMED_FIXTURE}.txt.gz"))
    assert header(fx.spec) == (29, 14, 3, 1, 0) and fx.list_sizes == [1]
    big = np.abs(fx.llr).max(axis=1)
    assert (big[:len(big) // 2] < 100.0).all() and (big[len(big) // 2:] > 1000.0).all() and big.max() < 100000.0


@pytest.mark.gpu
def test_gpu_shortened_named_code_matches_the_recorded_reference(kdir):
    """At L = 1 the compiled reference is defined for this code: its recorded lists
    (named_ref_A5_G_A_short, half of the rows with large LLRs), in the LDS state and the tiered
    one at every split, through the strict comparer."""
    fx = NL.fixture(os.path.join(NL.R.GOLD, f"named_ref_{short_codes.NAMED_FIXTURE}.txt.gz"))
    assert fx.spec == short_spec("A5_G_A")
    want = recorded_lists(fx, 1)
    for label, state, split in states(fx.spec, ("lds", "tiered_mixed")):
        with context(fx.spec, 1, state, split) as d:
            assert_strict(decode_host(d, fx.llr), want, f"A5_G_A {label} host")
            assert_strict(decode_device(d, fx.llr), want, f"A5_G_A {label} device")


@pytest.mark.gpu
@pytest.mark.parametrize("L,mode", [(1, "rounds"), (1, "items"), (4, "items")])
def test_gpu_shortened_search_layer_code_under_the_budget(L, mode, kdir, monkeypatch):
    """The 64 x 64 ordered-statistics search on a shortened code, suspended at every round (or
    item): the save / restore path carries the mapped LLRs, and the search's bounds round next to
    100000 as the oracle's do."""
    from test_polar_budget import TINY, _decode, _decoder
    spec = short_spec("bch64f")
    o = oracle(spec)
    info = np.random.default_rng(64 + L).integers(0, 2, (2, o.K)).astype(np.uint8)
    llr = awgn_llr(o.encode(info), 3.0, o.K / o.N, seed=64 + L)
    llr[1] *= short_codes.LARGE  # large LLRs, still below the shortened symbols' 100000 (see batches)
    assert 1000.0 < np.abs(llr[1]).max() < 100000.0
    want = o.decode_batch(llr, L)
    tiny = _decoder(monkeypatch, spec, L, kernel_dir(), TINY)
    try:
        if mode == "items":
            monkeypatch.setenv("BCHK_POLAR_NO_MID", "1")
        else:
            monkeypatch.delenv("BCHK_POLAR_NO_MID", raising=False)
        got = decode_host(tiny, llr)
        print(f"\nshortened bch64f L={L} {mode}: {tiny.last_launches()} launches")
        assert tiny.last_launches() > 1
        assert_strict(got, want, f"bch64f L={L} {mode}")
    finally:
        tiny.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arikan_n6", "arikan_n7", "bch16_A", "A_bch32f"])
def test_gpu_genie_on_a_shortened_code(name, kdir):
    """The genie kernel's LoadLLRs on shortened symbols: decision LLRs against the numpy
    restatement (tests/genie_lib.py) bit for bit, counters their column sums."""
    from test_polar_genie import Run
    spec = short_spec(name)
    g = GenieCode(spec, kernel_dir())
    with context(spec, 1) as d:
        info, cw, llr, err, soft, dec, u = Run(d, 48, seed=9).host()
    want_u = np.stack([g.build_u(w) for w in info])
    np.testing.assert_array_equal(u, want_u)
    want = np.stack([g.sc_llrs(llr[b], want_u[b]) for b in range(len(llr))])
    np.testing.assert_array_equal(dec.view(np.uint32), want.view(np.uint32))
    e, s = column_sums(want, want_u)
    np.testing.assert_array_equal(err.view(np.uint64), e)
    np.testing.assert_array_equal(soft, s)


# ================================================================ B. lists shorter than L

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHORT_LISTS))
def test_gpu_short_lists_leave_the_other_rows_and_the_guards(name, kdir, monkeypatch):
    """2^K < L: count = 2^K, rows past it untouched, through both entry points, in every state;
    70 words over 3 workgroups, which reuse their state from word to word."""
    monkeypatch.setenv("BCHK_POLAR_GRID", "3")
    build, L, count = SHORT_LISTS[name]
    spec = build()
    named = "G" in name
    o = oracle(spec)
    assert (1 << o.K) == count < L
    llr = batches(spec, 70, seed=11)[0]
    want = None if named else o.decode_batch(llr, L)
    for label, state, split in states(spec):
        with context(spec, L, state, split) as d:
            assert d.state_info()["grid"] == 3
            for how, fn in (("device", decode_device), ("host", decode_host)):
                got = fn(d, llr)
                what = f"{name} {label} {how}"
                assert (got[0] == count).all(), what
                if named and state == "lds":
                    named_contract(spec, got, what)
                    assert all(len({r.tobytes() for r in got[1][b, :count]}) == count for b in range(70))
                    want = want or got
                assert_strict(got, want, what)


# ================================================================ C. cw = NULL

# codes with N % 4 == 0, where the codeword rows take the 4-byte packed stores, besides the
# shortened ones (all of which have N % 4 != 0: byte stores)
NULL_CW_SPECS = {
    "A7-N128": lambda: arikan_spec(7, 64, dyn=4, seed=3),
    "A8-N256": lambda: arikan_spec(8, 128, dyn=3, seed=8 + 128),      # STORES' both-packed code
    "A6-N60": lambda: arikan_spec(6, 30, punct=(2, 9, 33, 50), seed=5),  # punctured onto a multiple of 4
    "bch16_A-N32": lambda: mixed_spec(("bch16", "A"), 16, 2, seed=5),
    "k3_k4_A-N24": lambda: mixed_spec(("k3", "k4", "A"), 12, 2, seed=7),
}
NULL_CW = [  # (state, code, split, L): a code of each state at N % 4 != 0 and at N % 4 == 0
    ("lds", "arikan_n6", None, 8), ("lds", "arikan_n7", None, 8),
    ("tiered", "arikan_n6", 2, 8), ("tiered", "arikan_n7", 7, 4),
    ("lds", "bch16_A", None, 8), ("lds", "k3_k4_A", None, 4),
    ("tiered_mixed", "bch16_A", 1, 4), ("tiered_mixed", "k3_k4_A", 3, 8), ("tiered_mixed", "A5_G_A", 2, 4),
    ("lds", "A7-N128", None, 8), ("lds", "A8-N256", None, 4), ("lds", "A6-N60", None, 8),
    ("tiered", "A7-N128", 3, 8), ("tiered", "A8-N256", 8, 4), ("tiered", "A6-N60", 1, 8),
    ("tiered_mixed", "A7-N128", 4, 4),
    ("lds", "bch16_A-N32", None, 8), ("lds", "k3_k4_A-N24", None, 4),
    ("tiered_mixed", "bch16_A-N32", 2, 4), ("tiered_mixed", "k3_k4_A-N24", 1, 8),
]


def test_cw_null_cases_cover_both_store_shapes():
    for state in ("lds", "tiered", "tiered_mixed"):
        names = [c[1] for c in NULL_CW if c[0] == state]
        assert any(n in NULL_CW_SPECS for n in names) and any(n in SHORT for n in names)
    for name, build in NULL_CW_SPECS.items():
        assert header(build())[0] % 4 == 0, name
    for name in SHORT:
        assert header(short_spec(name))[0] % 4 != 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("state,name,split,L", NULL_CW, ids=[f"{c[0]}-{c[1]}" for c in NULL_CW])
def test_gpu_cw_null(state, name, split, L, kdir):
    """d_cw = 0 / cw = NULL: count, info and metric as with a cw buffer, bit for bit, and a
    sentinel-filled buffer that is not passed stays as it is."""
    spec = NULL_CW_SPECS[name]() if name in NULL_CW_SPECS else short_spec(name)
    llr = batches(spec, seed=13)[1]
    with context(spec, L, state, split) as d:
        for fn in (decode_device, decode_host):
            full = fn(d, llr)
            assert_strict(fn(d, llr, cw=False), full, f"{name} {state} {fn.__name__}", cw=False)


@pytest.mark.gpu
def test_gpu_cw_null_under_the_budget(kdir, monkeypatch):
    from test_polar_budget import TINY, _decoder
    spec = short_spec("bch64f")
    o = oracle(spec)
    llr = awgn_llr(o.encode(np.ones((2, o.K), np.uint8)), 3.0, o.K / o.N, seed=3)
    monkeypatch.setenv("BCHK_POLAR_NO_MID", "1")
    d = _decoder(monkeypatch, spec, 1, kernel_dir(), TINY)
    try:
        full = decode_host(d, llr)
        assert_strict(full, o.decode_batch(llr, 1), "bch64f")
        assert_strict(decode_device(d, llr, cw=False), full, "bch64f cw = NULL", cw=False)
        assert d.last_launches() > 1
    finally:
        d.close()


# ================================================================ D. epilogue store shapes

STORES = [  # n, K, punctured: (K mod 4, N mod 4) zero / non-zero, K past a record word, a lane round
    (7, 33, ()),              # K % 4 != 0, N % 4 == 0; two record words
    (7, 67, (2, 90)),         # K % 4 != 0, N = 126; a second lane round of the byte stores
    (8, 130, (0, 77, 200)),   # K % 4 != 0, N = 253
    (8, 128, ()),             # both packed
    (8, 132, (5,)),           # K % 4 == 0 (packed info: 33 stores), N = 255 (byte codewords)
    (9, 264, ()),             # packed info past 64 lanes (66 stores), packed codewords past 64 lanes (128)
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,K,punct", STORES, ids=[f"A{c[0]}-K{c[1]}-N{(1 << c[0]) - len(c[2])}" for c in STORES])
@pytest.mark.parametrize("L", [1, 8])
def test_gpu_epilogue_store_shapes(n, K, punct, L, kdir):
    spec = arikan_spec(n, K, dyn=3, punct=punct, seed=n + K)
    key = f"stores-{n}-{K}"
    for label, state, split in states(spec, ("lds", "tiered")):
        check_against_oracle(key, spec, L, state, split, label)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EDGE_K))
def test_gpu_dimension_zero_and_nothing_frozen(name, kdir):
    """K = 0: one row, the frozen word, with the oracle's metric, and no information byte written;
    K = U at L = 8. Every state, both entry points."""
    build, L, count = EDGE_K[name]
    spec = build()
    llrs, wants = expected(name, spec, L)
    for label, state, split in states(spec):
        with context(spec, L, state, split) as d:
            for fn in (decode_host, decode_device):
                for i, (llr, want) in enumerate(zip(llrs, wants)):
                    got = fn(d, llr)
                    assert (got[0] == count).all()
                    assert_strict(got, want, f"{name} {label} {fn.__name__} batch {i}")


@pytest.mark.gpu
def test_gpu_dimension_zero_has_no_rate():
    """generate_device needs Eb/N0 -> sigma through K / N: refused before any launch."""
    F = load()
    with context(arikan_spec(4, 0), 4) as d:
        import torch
        t = torch.zeros(64, dtype=torch.float32, device="cuda:0")
        with pytest.raises(F.BchkError, match="dimension 0"):
            d.generate_device(1.0, 4, t.data_ptr())


# ================================================================ E. the device pipeline

PIPE = ["arikan_n7", "bch16_A"]
PIPE_SNR, PIPE_SEED, PIPE_B, PIPE_L = 1.0, 21, 64, 4


@functools.lru_cache(maxsize=None)
def pipe_ref(name):
    spec = short_spec(name)
    o = oracle(spec)
    info, cw, llr = P.polar_words(o.encode, o.N, o.K, PIPE_SNR, PIPE_SEED, 5, PIPE_B)
    return spec, o, info, cw, llr, P.llr_float32(llr)


@pytest.mark.parametrize("name", PIPE)
def test_pipeline_reference_has_no_undecidable_llr(name, kdir):
    spec, o, info, cw, llr, (f32, decidable) = pipe_ref(name)
    assert decidable.all()
    assert np.isclose(P.polar_sigma(o.N, o.K, PIPE_SNR) ** 2, 0.5 * 10 ** (-PIPE_SNR / 10) * o.N / o.K)
    assert o.N < o.U  # sigma from the transmitted length


@pytest.mark.gpu
@pytest.mark.parametrize("name", PIPE)
def test_gpu_pipeline_on_a_shortened_code(name, kdir):
    """encode_device against the oracle; generate_device against the Philox restatement, sigma
    from the transmitted N; count_device against the numpy counters; decode in between against
    the oracle."""
    import torch
    from test_polar_sim import Batch, _sync, _zeros, encode_device, generate, np_counters
    spec, o, info_ref, cw_ref, llr_ref, (f32, decidable) = pipe_ref(name)
    with context(spec, PIPE_L) as d:
        rnd = np.random.default_rng(3).integers(0, 2, (70, o.K)).astype(np.uint8)
        np.testing.assert_array_equal(encode_device(d, rnd), o.encode(rnd))
        np.testing.assert_array_equal(d.encode(rnd), o.encode(rnd))
        info, cw, llr = generate(d, PIPE_SNR, PIPE_B, seed=PIPE_SEED, word0=5)
        np.testing.assert_array_equal(info, info_ref)
        np.testing.assert_array_equal(cw, cw_ref)
        R = len(f32)
        np.testing.assert_array_equal(llr[:R].view(np.uint32), f32.view(np.uint32))
        bt = Batch(d, PIPE_SNR, PIPE_B, PIPE_SEED, word0=5)
        out8, flags = _zeros((8,), torch.int64), _zeros((PIPE_B,), torch.uint8)
        _sync()
        bt.count_device(0, PIPE_B, out8, flags)
        host = bt.host()
        np.testing.assert_array_equal(host[2].view(np.uint32), llr.view(np.uint32))
        cnt, inf, cws, _ = o.decode_batch(llr, PIPE_L)
        np.testing.assert_array_equal(host[5], cnt)
        for b in range(PIPE_B):
            np.testing.assert_array_equal(host[3][b, :cnt[b]], inf[b, :cnt[b]])
            np.testing.assert_array_equal(host[4][b, :cnt[b]], cws[b, :cnt[b]])
        per, want_flags = np_counters(*host)
        np.testing.assert_array_equal(out8.cpu().numpy(), per.sum(axis=0))
        np.testing.assert_array_equal(flags.cpu().numpy(), want_flags)
        assert per[:, 1].sum() > 0  # block errors occurred


@pytest.mark.gpu
@pytest.mark.parametrize("name", PIPE)
def test_gpu_sweep_on_a_shortened_code(name, kdir):
    """Two points, cut by errors, against generate + decode + count by hand."""
    from test_polar_sim import _reference_sweep
    spec = short_spec(name)
    with context(spec, PIPE_L) as d:
        recs, _, words = d.sweep_device(0.0, 1.0, 2, 600, 12, seed=PIPE_SEED, batch=100)
        want, last = _reference_sweep(d, 0.0, 1.0, 2, 600, 12, PIPE_SEED)
        assert recs == want
        assert all(c[1] == 12 and c[0] < 600 for _, c in recs), recs  # cut by errors
        assert words >= sum(c[0] for _, c in recs)


# ================================================================ F. genie on tiered contexts

GENIE = {
    "A7": (lambda: arikan_spec(7, 64, dyn=4, seed=3), ("tiered", "tiered_mixed")),
    "arikan_n6": (lambda: short_spec("arikan_n6"), ("tiered", "tiered_mixed")),
    "bch16_A": (lambda: mixed_spec(("bch16", "A"), 16, 2, seed=5), ("tiered_mixed",)),
    "A5_G_A": (lambda: NL.named_spec(("A5", "G", "A"), 15, seed=7, dyn=2), ("tiered_mixed",)),
}


def _genie(d, t_info, t_llr, B):
    import torch
    err = torch.zeros(d.U, dtype=torch.int64, device="cuda:0")
    soft = torch.zeros(d.U, dtype=torch.int64, device="cuda:0")
    dec = torch.zeros((B, d.U), dtype=torch.float32, device="cuda:0")
    u = torch.zeros((B, d.U), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    d.genie_device(t_info.data_ptr(), t_llr.data_ptr(), B, err.data_ptr(), soft.data_ptr(), dec.data_ptr(), u.data_ptr())
    d.sync()
    return tuple(t.cpu().numpy() for t in (err, soft, dec, u))


def _same_bits(got, want, what):
    for g, w in zip(got, want):
        g, w = (a.view(np.uint32) if a.dtype == np.float32 else a for a in (g, w))
        np.testing.assert_array_equal(g, w, err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENIE))
def test_gpu_genie_on_tiered_contexts(name, kdir):
    """genie_device's decision LLRs, u rows and counters, and genie_run's totals, on contexts
    created tiered at split 1 and split = layers: those of an LDS-state context of the same
    specification (pinned by tests/test_polar_genie.py and test A above). Then a decode and a
    genie_run interleaved on the tiered context, which share its buffers."""
    import torch
    build, kinds = GENIE[name]
    spec = build()
    B, L = 48, 4
    with context(spec, L) as d:
        t_info = torch.zeros((B, d.K), dtype=torch.uint8, device="cuda:0")
        t_llr = torch.zeros((B, d.N), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        d.generate_device(2.0, B, t_llr.data_ptr(), t_info.data_ptr(), seed=5)
        d.sync()
        want = _genie(d, t_info, t_llr, B)
        want_run = d.genie_run(2.0, 100, seed=5, batch=37)[:2]
        llr = t_llr.cpu().numpy()
        want_lists = decode_host(d, llr)
    assert want[0].sum() > 0  # decision errors occurred
    for kind in kinds:
        for split in (1, n_layers(spec)):
            what = f"{name} {kind} split {split}"
            with context(spec, L, kind, split) as d:
                _same_bits(_genie(d, t_info, t_llr, B), want, what)
                _same_bits(d.genie_run(2.0, 100, seed=5, batch=37)[:2], want_run, what)
                assert_strict(decode_host(d, llr), want_lists, what)
                _same_bits(d.genie_run(2.0, 100, seed=5)[:2], want_run, what)
                assert_strict(decode_device(d, llr), want_lists, what)
                _same_bits(_genie(d, t_info, t_llr, B), want, what)
