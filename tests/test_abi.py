"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports
exactly what include/bchk.h declares; without a GPU it fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import pytest

from bchk_pkg import REPO, load


def header_symbols():
    src = open(os.path.join(REPO, "include", "bchk.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bchk_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_binding_exports():
    assert header_symbols() == sorted(load().EXPORTS)


def test_library_exports_every_declared_symbol():
    bchk = load()
    path = bchk.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (bchk_[a-z0-9_]+)$", out, flags=re.M))
    missing = set(header_symbols()) - exported
    assert not missing, missing
    lib = ctypes.CDLL(path)
    for s in header_symbols():
        assert hasattr(lib, s)


def test_library_has_gfx950_code_object():
    data = open(load().build(), "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data


def test_create_fails_loudly_without_gpu():
    bchk = load()
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(bchk.BchkError, match="device|HIP"):
        bchk.KanekoKernelProcessor(6, 6)


def test_invalid_code_parameters_rejected():
    bchk = load()
    for m, t in ((1, 1), (9, 2), (4, 8), (6, 0)):
        with pytest.raises(bchk.BchkError):
            bchk.KanekoKernelProcessor(m, t)


def dispatch_groups():
    """Every (m, t) bchk_create accepts, grouped by what bchk_kernel_info reports for it."""
    bchk = load()
    groups = {}
    for m in range(2, 9):
        for t in range(1, min(1 << (m - 1), 33)):
            info = bchk.kernel_info(m, t)
            groups.setdefault((m,) + tuple(info[f] for f in bchk.KERNEL_INFO_FIELDS), []).append(t)
    return groups


def test_kernel_info_refuses_what_create_refuses():
    bchk = load()
    for m, t in ((1, 1), (9, 2), (2, 2), (3, 4), (4, 8), (5, 16), (6, 0), (6, 32), (7, 33), (8, 33), (8, -1)):
        with pytest.raises(bchk.BchkError):
            bchk.kernel_info(m, t)
    # the shapes the design documents: no fast kernel at m = 2 or above the fast buckets, a lane
    # pre-pass only in <7,8> and <8,15>, no selection first kernel at TMAX = 32, no table past t = 7
    assert bchk.kernel_info(2, 1) == dict(tmax=1, fast=0, lane=0, selection=0, table=1, tail=1)
    assert bchk.kernel_info(6, 7) == dict(tmax=12, fast=0, lane=0, selection=0, table=0, tail=0)
    assert bchk.kernel_info(8, 15) == dict(tmax=15, fast=1, lane=1, selection=1, table=0, tail=0)
    assert bchk.kernel_info(8, 16) == dict(tmax=16, fast=1, lane=0, selection=1, table=0, tail=0)
    assert bchk.kernel_info(7, 32) == dict(tmax=32, fast=1, lane=0, selection=0, table=0, tail=0)


def test_every_dispatch_group_has_a_gpu_parity_case():
    # test_bucket_parity.CASES holds, per group, at least the lowest t, the top t and (three or
    # more t) one t inside: a kernel set or a new combination of stages without cases fails
    # here, on any machine, and so does taking out a group's lowest, top or only inner case
    from test_bucket_parity import CASES, TOP_INSTEAD
    cases = sorted({(m, t) for m, t, *_ in CASES})
    assert len(cases) == len(CASES)
    bchk = load()
    covered = {}
    for m, t in cases:
        info = bchk.kernel_info(m, t)
        covered.setdefault((m,) + tuple(info[f] for f in bchk.KERNEL_INFO_FIELDS), []).append(t)
    groups = dispatch_groups()
    assert len(groups) >= 16 and set(covered) <= set(groups)
    for g, ts in groups.items():
        assert g in covered, f"no GPU parity case for dispatch group {g} (t = {ts})"
        ends = [ts[0], TOP_INSTEAD.get((g[0], ts[-1]), ts[-1])]
        got = covered[g]
        assert set(ends) <= set(got), f"dispatch group {g}: cases at t = {got}, wanted {ends}"
        inner = [t for t in got if ends[0] < t < ends[1]]
        assert len(inner) >= (1 if len(ts) >= 3 else 0), (g, got)
