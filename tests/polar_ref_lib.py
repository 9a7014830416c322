"""The tests/golden/polar_ref_*.txt.gz fixtures: inputs and RECORDED OUTPUTS of the reference's
vendored polar library itself (its SC-list decoder, encoder, trellis kernel processor with its
operation counters, kernel-file reader and BEC capacity evaluator),
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
  @lu_code c       (no lines) the kernel is the field-ordered 16 x 16 extended-BCH kernel with
                   its columns mapped by candidate code c of the column search
  @counts_in       channel LLR rows, f32 hex                         (column-search score input)
  @counts_out      polar_ref's stdout: per row '<SumCount growth> <CmpCount growth>' over GetLLRs
                   at every phase in order, zero known inputs (root bchCoder.cpp:641-653)
  @kernel_file F   kernel file F, its text line by line exactly as bchk_kernel_write_file wrote
                   it: size, matrix, '3', the BEC table (Kernel.cpp:93-134)
  @capacity_in     channel capacities, one per line, f64 as hex bits
  @capacity_out    polar_ref's stdout: per capacity GetSubchannelCapacity(ec_BEC, phase, .) of
                   every phase, f64 hex bits (CapacityEvaluator.cpp:124-140, NaN and -inf included)
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
    """kind 'code' (decoder + encoder fixtures), 'trellis', 'counts' or 'capacity'."""
    all_ = sorted(glob.glob(os.path.join(GOLD, "polar_ref_*.txt.gz")))
    by = {k: [p for p in all_ if os.path.basename(p).startswith(f"polar_ref_{k}_")] for k in ("trellis", "counts", "capacity")}
    return by[kind] if kind in by else [p for p in all_ if not any(p in v for v in by.values())]


def hex_row(a):
    return " ".join(f"{int(x):08x}" for x in np.ascontiguousarray(a, np.float32).view(np.uint32))


def hex64(v):
    return f"{int(np.float64(v).view(np.uint64)):016x}"


def f64_row(line):
    return np.array([int(w, 16) for w in line.split()], np.uint64).view(np.float64)


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

    @property
    def kernel_file(self):
        """(name, text) of the fixture's '@kernel_file' section."""
        for n, a, lines in self.sections:
            if n == "kernel_file":
                return a[0], "\n".join(lines) + "\n"
        raise KeyError("kernel_file")

    @property
    def counts(self):
        """(y f32 [rows][l], [(Sum, Cmp)] per row)."""
        y = np.array([[int(w, 16) for w in r.split()] for r in self.get("counts_in")], np.uint32).view(np.float32)
        return y, [tuple(int(v) for v in r.split()) for r in self.get("counts_out")]

    @property
    def lu_code(self):
        for n, a, _ in self.sections:
            if n == "lu_code":
                return int(a[0])
        return None

    def write_kernels(self, d):
        for fname, K in self.kernels.items():
            with open(os.path.join(d, fname), "w") as f:
                f.write(kernel_text(K))
        if self.has("kernel_file"):
            fname, text = self.kernel_file
            with open(os.path.join(d, fname), "w") as f:
                f.write(text)

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


_modes = {}


def ref_lacks(mode, binary=POLAR_REF):
    """Why a regeneration test of `mode` cannot run, or None. The binary names its modes in its
    usage line (no arguments: exit 2); one built from a driver older than the mode does not name
    it, and is as good as absent for that mode."""
    if not os.path.exists(binary):
        return "oracle/_ref/polar_ref is not built (the reference tree is absent)"
    if binary not in _modes:
        r = subprocess.run([binary], capture_output=True, text=True, stdin=subprocess.DEVNULL)
        _modes[binary] = r.stderr
    if f" {mode} " not in _modes[binary]:
        return f"oracle/_ref/polar_ref was built from a driver without the `{mode}` mode (rebuild: make -C oracle ref)"
    return None


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
        elif n == "counts_out":
            (kfile,) = fx.kernels.keys()
            lines = run_ref(["counts", kfile], fx.get("counts_in"), workdir, binary)
        elif n == "capacity_out":
            lines = run_ref(["capacity", fx.kernel_file[0]], fx.get("capacity_in"), workdir, binary)
        out.sections.append((n, a, lines))
    return out
