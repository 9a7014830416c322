"""The tests/golden/polar_ref_*.txt.gz fixtures: inputs and RECORDED OUTPUTS of the reference's
vendored polar library itself (its SC-list decoder, encoder and trellis kernel processor),
compiled into oracle/_ref/polar_ref by oracle/Makefile and run by `oracle/make_golden.py
polar`. Data only. Shared by that generator and tests/test_polar_reference.py.

A fixture is gzip text: '#' comment lines, then sections '@name [args] <nlines>' each followed
by its nlines lines:
  @spec            the code specification text (MixedKernelEncoder.cpp:7-98)
  @kernel F l      kernel file F: l rows of l 0/1 entries (Kernel.cpp:93-107)
  @llr             channel LLR rows, one per line, f32 as hex bits   (decoder input)
  @decode L        polar_ref's stdout for those rows at list size L: per row 'D <count>' and
                   count lines '<info bits> <codeword bits> <metric f32 hex>', list order
  @info            information words, one per line                   (encoder input)
  @encode          polar_ref's stdout for those words: codeword bits
  @trellis_in      per line '<u bits> <y f32 hex ...>'               (kernel processor input)
  @trellis_out     polar_ref's stdout: per line the l kernel-input LLRs (phase p given
                   u_0..u_{p-1}), f32 hex
"""
import glob
import gzip
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
POLAR_REF = os.path.join(REPO, "oracle", "_ref", "polar_ref")


def fixture_files(kind):
    """kind 'code' (decoder + encoder fixtures) or 'trellis'."""
    all_ = sorted(glob.glob(os.path.join(GOLD, "polar_ref_*.txt.gz")))
    tr = [p for p in all_ if os.path.basename(p).startswith("polar_ref_trellis_")]
    return tr if kind == "trellis" else [p for p in all_ if p not in tr]


def hex_row(a):
    return " ".join(f"{int(x):08x}" for x in np.ascontiguousarray(a, np.float32).view(np.uint32))


def bits_row(a):
    return "".join("1" if v else "0" for v in a)


def bits(s):
    return np.frombuffer(s.encode(), np.uint8) - ord("0")


def kernel_text(K):
    return f"{len(K)}\n" + "\n".join(" ".join(str(int(v)) for v in row) for row in K) + "\n"


class Fixture:
    def __init__(self, name, comments=()):
        self.name = name
        self.comments = list(comments)
        self.sections = []  # (name, args, lines)

    def add(self, name, args, lines):
        self.sections.append((name, [str(a) for a in args], list(lines)))

    def get(self, name, *args):
        want = [str(a) for a in args]
        for n, a, lines in self.sections:
            if n == name and a[:len(want)] == want:
                return lines
        raise KeyError((name, args))

    def has(self, name):
        return any(n == name for n, _, _ in self.sections)

    # ---- typed views
    @property
    def spec(self):
        return "\n".join(self.get("spec")) + "\n"

    @property
    def kernels(self):
        out = {}
        for n, a, lines in self.sections:
            if n == "kernel":
                out[a[0]] = np.array([[int(v) for v in r.split()] for r in lines], np.uint8)
        return out

    @property
    def list_sizes(self):
        return [int(a[0]) for n, a, _ in self.sections if n == "decode"]

    @property
    def llr(self):
        rows = [[int(w, 16) for w in r.split()] for r in self.get("llr")]
        return np.array(rows, np.uint32).view(np.float32)

    @property
    def info(self):
        return np.array([bits(r) for r in self.get("info")], np.uint8)

    @property
    def encoded(self):
        return np.array([bits(r) for r in self.get("encode")], np.uint8)

    def decoded(self, L):
        """[(count, info [count][K], codewords [count][N], metric bits u32 [count])] per row."""
        out, lines, i = [], self.get("decode", L), 0
        while i < len(lines):
            tag, c = lines[i].split()
            assert tag == "D"
            c = int(c)
            ent = [r.split() for r in lines[i + 1:i + 1 + c]]
            out.append((c, np.array([bits(e[0]) for e in ent], np.uint8),
                        np.array([bits(e[1]) for e in ent], np.uint8),
                        np.array([int(e[2], 16) for e in ent], np.uint32)))
            i += 1 + c
        return out

    def write_kernels(self, d):
        for fname, K in self.kernels.items():
            with open(os.path.join(d, fname), "w") as f:
                f.write(kernel_text(K))

    # ---- file form
    def dumps(self):
        out = ["# " + c for c in self.comments]
        for n, a, lines in self.sections:
            out.append(" ".join(["@" + n] + a + [str(len(lines))]))
            out.extend(lines)
        return "\n".join(out) + "\n"

    def save(self, path):
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
            f.write(self.dumps().encode())


def load_fixture(path):
    with gzip.open(path, "rt") as f:
        lines = f.read().split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    fx = Fixture(os.path.basename(path)[len("polar_ref_"):-len(".txt.gz")])
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("#"):
            fx.comments.append(ln[2:])
            i += 1
            continue
        assert ln.startswith("@"), ln
        p = ln[1:].split()
        n = int(p[-1])
        fx.sections.append((p[0], p[1:-1], lines[i + 1:i + 1 + n]))
        i += 1 + n
    return fx


def run_ref(args, stdin_lines, cwd, binary=POLAR_REF):
    r = subprocess.run([binary] + [str(a) for a in args], input="\n".join(stdin_lines) + "\n",
                       capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        raise RuntimeError(f"polar_ref {args}: exit {r.returncode}: {r.stderr.strip()[-2000:]}")
    return r.stdout.split("\n")[:-1]


def regenerate(fx, workdir, binary=POLAR_REF):
    """Run the reference binary on the fixture's inputs: a Fixture with the same inputs and
    freshly computed output sections."""
    out = Fixture(fx.name, fx.comments)
    fx.write_kernels(workdir)
    if fx.has("spec"):
        with open(os.path.join(workdir, "spec.txt"), "w") as f:
            f.write(fx.spec)
    for n, a, lines in fx.sections:
        if n == "decode":
            lines = run_ref(["decode", "spec.txt", a[0]], fx.get("llr"), workdir, binary)
        elif n == "encode":
            lines = run_ref(["encode", "spec.txt"], fx.get("info"), workdir, binary)
        elif n == "trellis_out":
            (kfile,) = fx.kernels.keys()
            lines = run_ref(["trellis", kfile], fx.get("trellis_in"), workdir, binary)
        out.sections.append((n, a, lines))
    return out
