"""Dense dynamic freezing, the host side (no GPU): the codes of tests/dense_codes.py are what they
claim; the mask holds 64 live constraints and every entry point refuses the 65th with the
reference's message; and the C oracle, which restates the library's mask scheme, agrees bit for bit
with a decoder that has no mask at all (tests/sclist_plain.py: whole u vectors, a frozen symbol the
XOR of its listed terms) on the two dense Arikan codes. The GPU half is tests/test_polar_dense_dyn.py.
"""
import ctypes as C

import numpy as np
import pytest

import dense_codes
import sclist_plain
from bchk_pkg import load
from polar_lib import (ARIKAN, PolarOracle, awgn_llr, constraint_bits, correction_words, dense_arikan_spec,
                       kernel_transform, max_active, spec_constraints, spec_inputs)
from test_polar_mixed import KERNELS, kdir  # noqa: F401

ALL = list(dense_codes.ARIKAN) + list(dense_codes.MIXED)
WIDE = [n for n in ALL if (dense_codes.ARIKAN.get(n) or dense_codes.MIXED[n]).get("widths")]
TOO_MANY = "Too many dynamic freezing constraints are simultaneously active"


def matrices(name):
    return [ARIKAN if l == "A" else KERNELS[l] for l in dense_codes.layers(name)]


def direct_encode(name, info):
    """Codewords from the specification text alone: frozen symbols by XOR of their terms."""
    spec = dense_codes.spec(name)
    U = int(np.prod([len(M) for M in matrices(name)]))
    return kernel_transform(spec_inputs(spec, U, info), matrices(name))


# ---------------------------------------------------------------- the specs

@pytest.mark.parametrize("name", ALL)
def test_dense_spec_is_what_its_name_claims(name):
    spec = dense_codes.spec(name)
    par = dict(dense_codes.ARIKAN.get(name) or dense_codes.MIXED[name])
    active, pivot, late = dense_codes.claimed_active(name), par["pivot"], par.get("late", 0)
    assert par["active"] == active > 32
    cons = spec_constraints(spec)
    frozen = {c[-1] for c in cons}
    dyn = [c for c in cons if len(c) > 1]
    assert max_active(spec) == active and len(dyn) == active + late
    across = [c for c in dyn if c[0] < pivot]
    assert len(across) == active
    for c in across:  # first term below the pivot, frozen symbol at or above it, information symbols in between
        assert c[-1] >= pivot and c == sorted(c) and not frozen & set(c[:-1])
    bit = constraint_bits(spec)
    assert sorted(bit[c[-1]] for c in across) == list(range(active))  # bit active - 1 is in use
    # the late ones start past the pivot on bits that others have given back
    assert all(c[0] >= pivot and bit[c[-1]] < active for c in dyn if c not in across)
    assert (late > 0) == (len(set(bit.values())) < len(bit))
    lengths = {len(c) for c in dyn}
    assert {2, 3} <= lengths  # a plain copy, the usual three
    if name in WIDE:  # 65 terms and the symbol; more than 128 terms
        assert 66 in lengths and max(lengths) > 129
    # one information symbol in 20 or more constraints, its correction word in both halves of the mask
    corr = correction_words(spec)
    uses = {s: sum(s in c[:-1] for c in dyn) for s in corr if s not in frozen}
    hub = max(uses, key=uses.get)
    assert uses[hub] >= 20 and corr[hub] & 0xFFFFFFFF and corr[hub] >> 32 and corr[hub] != (1 << active) - 1


def test_helpers_on_a_hand_made_spec():
    # symbols:   0 i, 1 i, 2 = u0, 3 i, 4 = u1 + u3, 5 = u3, 6 i, 7 = u6
    spec = "8 4 0 3 0 0\nA A A\n2 0 2\n3 1 3 4\n2 3 5\n2 6 7\n"
    assert max_active(spec) == 2  # (0, 2) and (1, 4) at symbol 1; (1, 4) and (3, 5) at symbol 3
    assert constraint_bits(spec) == {2: 0, 4: 1, 5: 0, 7: 0}
    assert correction_words(spec) == {0: 1, 2: 1, 1: 2, 3: 2 | 1, 4: 2, 5: 1, 6: 1, 7: 1}
    u = spec_inputs(spec, 8, np.array([[1, 0, 1, 1], [0, 1, 1, 0]], np.uint8))
    np.testing.assert_array_equal(u, [[1, 0, 1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 0, 1, 0, 0]])
    np.testing.assert_array_equal(kernel_transform(u, [ARIKAN] * 3), PolarOracle(spec).encode([[1, 0, 1, 1], [0, 1, 1, 0]]))
    np.testing.assert_array_equal(sclist_plain.encode(u[0]), kernel_transform(u[:1], [ARIKAN] * 3)[0])


# ---------------------------------------------------------------- the limit

def test_64_live_constraints_are_accepted_and_the_65th_is_refused():
    """Every create entry point parses before it touches the device: a code with 64 live constraints
    passes the parser (without a GPU what is left to fail is the device), one with 65 is refused
    with the reference's message (KernelListEngine.cpp:28), by the oracle too."""
    import torch
    F = load()
    lib = F.lib()
    full, over = dense_codes.spec("dyn_arikan_n8_a64"), dense_arikan_spec(**dense_codes.OVER)
    assert max_active(full) == 64 and max_active(over) == 65
    with pytest.raises(ValueError, match="more than 64"):
        constraint_bits(over)
    PolarOracle(full)
    with pytest.raises(ValueError, match=TOO_MANY):
        PolarOracle(over)
    creators = {
        "create": lambda s, h: lib.bchk_polar_create(s, 4, 0, C.byref(h)),
        "create_kdir": lambda s, h: lib.bchk_polar_create_kdir(s, None, 4, 0, C.byref(h)),
        "create_tiered": lambda s, h: lib.bchk_polar_create_tiered(s, None, 4, 0, -1, C.byref(h)),
        "create_tiered_mixed": lambda s, h: lib.bchk_polar_create_tiered_mixed(s, None, 4, 0, -1, C.byref(h)),
    }
    for what, create in creators.items():
        h = C.c_void_p()
        assert create(over.encode(), h) != 0 and not h.value, what
        assert TOO_MANY in lib.bchk_last_error().decode(), what
        h = C.c_void_p()
        rc = create(full.encode(), h)
        if torch.cuda.is_available():
            assert rc == 0 and h.value, (what, lib.bchk_last_error().decode())
            lib.bchk_polar_destroy(h)
        else:
            msg = lib.bchk_last_error().decode()
            assert rc != 0 and TOO_MANY not in msg and ("device" in msg or "HIP" in msg or "hip" in msg), (what, msg)


# ---------------------------------------------------------------- the oracle from first principles

@pytest.mark.parametrize("name", ALL)
def test_oracle_encoder_is_the_direct_xor_of_terms(name, kdir):
    o = PolarOracle(dense_codes.spec(name), kdir)
    info = np.random.default_rng(len(name)).integers(0, 2, (24, o.K)).astype(np.uint8)
    np.testing.assert_array_equal(o.encode(info), direct_encode(name, info))


_words = {}


def plain_workload(name):
    """16 received words per dense Arikan code, seed 4242 (the fixtures' are 2000 ..)."""
    if name not in _words:
        spec = dense_codes.spec(name)
        o = PolarOracle(spec)
        info = np.random.default_rng(4242).integers(0, 2, (16, o.K)).astype(np.uint8)
        _words[name] = spec, o, awgn_llr(o.encode(info), 1.0, o.K / o.N, seed=4243)
    return _words[name]


@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("name", ["dyn_arikan_n8_a64", "dyn_arikan_n7_a33"])
def test_oracle_matches_the_plain_decoder(name, L):
    spec, o, llr = plain_workload(name)
    cnt, info, cw, met = o.decode_batch(llr, L)
    diverged = False
    for b in range(len(llr)):
        c, pi, pw, pm = sclist_plain.decode(spec, llr[b], L)
        assert c == cnt[b], f"list count, row {b}"
        np.testing.assert_array_equal(info[b, :c], pi, err_msg=f"information vectors, row {b}")
        np.testing.assert_array_equal(cw[b, :c], pw, err_msg=f"codewords, row {b}")
        np.testing.assert_array_equal(met[b, :c].view(np.uint32), pm.view(np.uint32), err_msg=f"metric bits, row {b}")
        # every list entry is a codeword of the code: its information vector encodes to it
        np.testing.assert_array_equal(direct_encode(name, pi), pw, err_msg=f"re-encoded list, row {b}")
        diverged = diverged or len({m for m in pm.tolist()}) > 1
    assert diverged == (L > 1)
