"""bchk_amd -- Python view of libbchk.so (MI355X Kaneko/BCH soft decoder), via ctypes.

The product is the C ABI in include/bchk.h (HIP kernels for gfx950 + C++ host runtime);
this module only marshals numpy arrays / device pointers for tests, bench.py and
__graft_entry__. It mirrors the reference's KanekoKernelProcessor / Decoder / fun()
surface (headers/KanekoKernelProcessor.h:47-68, headers/Decoder.h:67-78,
headers/dataForPlot.h:8) with batched calls. There is no CPU fallback: if the HIP library
or a gfx950 device is missing, constructing a KanekoKernelProcessor raises.

Load it by path (the directory name is not an identifier):
    spec = importlib.util.spec_from_file_location("bchk_amd", ".../__init__.py")
"""
import ctypes as C
import math
import numbers
import os
import subprocess
import sys

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
# BCHK_LIB selects another build of the same ABI (e.g. lib/libbchk_diag.so)
LIB_PATH = os.environ.get("BCHK_LIB") or os.path.join(PKG_DIR, "lib", "libbchk.so")

BCHK_J_SHIPPED = -1
VARIANT_ANSWER, VARIANT_WORD = 0, 1
F_ACCEPTED, F_RETURNED, F_TRUNCATED, F_TIE, F_SCAN_UB = 1, 2, 4, 8, 16

# Every exported entry point of include/bchk.h.
EXPORTS = (
    "bchk_create", "bchk_destroy", "bchk_code_params", "bchk_generator",
    "bchk_set_max_decodes", "bchk_decode_host", "bchk_decode_device",
    "bchk_decode_variant_host", "bchk_alg_decode_host", "bchk_count_device", "bchk_decode_count_device",
    "bchk_generate_host", "bchk_generate_host_draws", "bchk_generate_device", "bchk_sweep_device", "bchk_rng_jump", "bchk_sweep_block", "bchk_sweep_range", "bchk_stream_skip",
    "bchk_stream_sync", "bchk_sweep", "bchk_sync", "bchk_stream", "bchk_profile",
    "bchk_profile_read", "bchk_profile_read_stages", "bchk_path_counts", "bchk_tail_count",
    "bchk_tail_stats", "bchk_coop_stats", "bchk_tail_diag_read", "bchk_tail_prof_read", "bchk_set_fast_path", "bchk_set_analytic",
    "bchk_set_chunk_limit", "bchk_set_syndrome_table", "bchk_first_pass_waves",
    "bchk_syndrome_table_query", "bchk_syndrome_table_info", "bchk_kernel_info", "bchk_polar_create", "bchk_polar_create_kdir",
    "bchk_polar_destroy", "bchk_polar_params", "bchk_polar_decode_host", "bchk_polar_decode_device",
    "bchk_polar_encode_host", "bchk_polar_sync", "bchk_polar_stream", "bchk_polar_last_launches",
    "bchk_polar_scratch_bytes", "bchk_polar_encode_device", "bchk_polar_generate_device",
    "bchk_polar_count_device", "bchk_polar_sweep_device", "bchk_polar_create_tiered", "bchk_polar_create_tiered_mixed",
    "bchk_polar_state_info",
    "bchk_kernel_ebch", "bchk_kernel_field_order", "bchk_kernel_trellis_cost", "bchk_kernel_column_costs",
    "bchk_kernel_column_search",
    "bchk_kernel_bec_masks", "bchk_kernel_bec_behaviour", "bchk_kernel_bec_sample", "bchk_kernel_bec_capacity",
    "bchk_kernel_write_file", "bchk_polar_design_bec", "bchk_polar_genie_device", "bchk_polar_genie_run",
    "bchk_polar_design_genie", "bchk_polar_generate_channel_device", "bchk_polar_sweep_channel_device",
    "bchk_polar_genie_run_channel", "bchk_polar_design_genie_channel",
    "bchk_polar_create_q8", "bchk_polar_create_q8_tiered", "bchk_polar_decode_q8_host", "bchk_polar_decode_q8_device",
    "bchk_polar_quantize_device", "bchk_polar_sweep_q8_device",
    "bchk_polar_generate_fading_device", "bchk_polar_sweep_fading_device", "bchk_polar_genie_run_fading",
    "bchk_polar_design_genie_fading", "bchk_polar_sweep_q8_fading_device", "bchk_last_error", "bchk_version",
)

# BCHK_CHANNEL_*: the channels of the polar simulation front-end
CHANNEL_AWGN, CHANNEL_RAYLEIGH, CHANNEL_BSC = 0, 1, 2
CHANNELS = {"awgn": CHANNEL_AWGN, "rayleigh": CHANNEL_RAYLEIGH, "bsc": CHANNEL_BSC}
# BCHK_FADING_*: the fading models with a parameter (FadingChannel)
FADING_BLOCK, FADING_CORRELATED, FADING_RICIAN = 0, 1, 2
FADINGS = {"rayleigh_block": FADING_BLOCK, "rayleigh_correlated": FADING_CORRELATED, "rician": FADING_RICIAN}

# struct bchk_polar_point: one Eb/N0 point of PolarListDecoder.sweep_device (on the BSC snr_db holds p)
POLAR_POINT_DTYPE = np.dtype([("snr_db", "<f8"), ("c", "<u8", (8,))])
POLAR_COUNTERS = ("words", "block_errors", "info_bit_errors", "code_bit_errors", "ml_errors", "list_errors",
                  "raw_bit_errors", "no_decision")

STATS_DTYPE = np.dtype([("decodes", "<u8"), ("comparisons", "<u8"), ("sums", "<u8"),
                        ("iterations", "<u8"), ("jsteps", "<u8"), ("improvements", "<u8"),
                        ("flags", "<u4"), ("reserved", "<u4")])


class BchkError(RuntimeError):
    pass


def build(force=False):
    """Compile libbchk.so in-tree (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(LIB_PATH):
        jobs = os.environ.get("MAX_JOBS", "8")
        subprocess.run(["make", "-s", "-C", PKG_DIR, f"-j{min(int(jobs), 16)}"], check=True)
    return LIB_PATH


_lib = None


def lib():
    """Load libbchk.so. If torch is importable it is imported first so that one HIP
    runtime (torch's libamdhip64.so.7) serves both torch and libbchk in this process."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BchkError(f"{LIB_PATH} missing: run make -C {PKG_DIR} (no CPU fallback)")
    if "torch" not in sys.modules and os.environ.get("BCHK_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32, u64, dbl = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_double
    L.bchk_create.argtypes = [i32, i32, i32, dbl, i32, C.POINTER(vp)]
    L.bchk_destroy.argtypes = [vp]
    L.bchk_destroy.restype = None
    L.bchk_code_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.bchk_generator.argtypes = [vp, vp]
    L.bchk_set_max_decodes.argtypes = [vp, u64]
    L.bchk_decode_host.argtypes = [vp, vp, sz, vp, vp, vp]
    L.bchk_decode_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.bchk_decode_variant_host.argtypes = [vp, i32, vp, sz, vp, vp, vp]
    L.bchk_alg_decode_host.argtypes = [vp, vp, vp, sz, vp, vp]
    L.bchk_count_device.argtypes = [vp, vp, vp, vp, sz, vp, vp]
    L.bchk_decode_count_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.bchk_generate_device.argtypes = [vp, C.c_double, sz, u64, u64, vp, vp, vp]
    L.bchk_sweep_device.argtypes = [vp, C.c_long, C.c_long, C.c_double, u64, sz, C.c_char_p, sz,
                                    C.POINTER(C.c_double), C.POINTER(u64)]
    L.bchk_generate_host.argtypes = [vp, dbl, sz, C.POINTER(u64), u64, vp, vp]
    L.bchk_generate_host_draws.argtypes = [vp, dbl, sz, C.POINTER(u64), u64, vp, vp, C.POINTER(u64)]
    L.bchk_rng_jump.argtypes = [u64, u64]
    L.bchk_rng_jump.restype = u64
    L.bchk_sweep_block.argtypes = [vp, dbl, C.POINTER(u64), sz, sz, vp, vp, vp, vp, vp]
    L.bchk_sweep_range.argtypes = [vp, dbl, C.POINTER(u64), u64, sz, vp, vp, vp, vp, vp, C.POINTER(sz)]
    L.bchk_stream_skip.argtypes = [i32, i32, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.bchk_stream_sync.argtypes = [i32, i32, u64, u64, u64, C.POINTER(u64), C.POINTER(u64)]
    L.bchk_sweep.argtypes = [vp, C.c_long, C.c_long, dbl, C.POINTER(u64), u64, sz, C.c_char_p, sz]
    L.bchk_sync.argtypes = [vp]
    L.bchk_stream.argtypes = [vp]
    L.bchk_stream.restype = vp
    L.bchk_profile.argtypes = [vp, i32]
    L.bchk_profile_read.argtypes = [vp, C.POINTER(dbl), C.POINTER(u64)]
    L.bchk_set_fast_path.argtypes = [vp, i32]
    L.bchk_set_syndrome_table.argtypes = [vp, i32]
    L.bchk_first_pass_waves.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.bchk_polar_create.argtypes = [C.c_char_p, i32, i32, C.POINTER(vp)]
    L.bchk_polar_create_kdir.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.POINTER(vp)]
    L.bchk_polar_create_tiered.argtypes = [C.c_char_p, C.c_char_p, i32, i32, i32, C.POINTER(vp)]
    L.bchk_polar_create_tiered_mixed.argtypes = [C.c_char_p, C.c_char_p, i32, i32, i32, C.POINTER(vp)]
    L.bchk_polar_state_info.argtypes = [vp, C.POINTER(i32), C.POINTER(u64), C.POINTER(u64), C.POINTER(i32)]
    L.bchk_polar_destroy.argtypes = [vp]
    L.bchk_polar_destroy.restype = None
    L.bchk_polar_params.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.bchk_polar_decode_host.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.bchk_polar_decode_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.bchk_polar_encode_host.argtypes = [vp, vp, sz, vp]
    L.bchk_polar_sync.argtypes = [vp]
    L.bchk_polar_stream.argtypes = [vp]
    L.bchk_polar_stream.restype = vp
    L.bchk_polar_scratch_bytes.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.bchk_polar_encode_device.argtypes = [vp, vp, sz, vp, vp]
    L.bchk_polar_generate_device.argtypes = [vp, dbl, sz, u64, u64, vp, vp, vp, vp]
    L.bchk_polar_count_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp]
    L.bchk_polar_sweep_device.argtypes = [vp, dbl, dbl, i32, u64, u64, u64, sz, vp, C.POINTER(dbl),
                                          C.POINTER(u64)]
    L.bchk_syndrome_table_query.argtypes = [i32, i32, vp, sz, vp, vp]
    L.bchk_syndrome_table_info.argtypes = [i32, i32, C.POINTER(u64), C.POINTER(u64),
                                           C.POINTER(C.c_uint32)]
    L.bchk_kernel_info.argtypes = [i32, i32, C.POINTER(C.c_int32)]
    L.bchk_path_counts.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.bchk_tail_count.argtypes = [vp, C.POINTER(u64)]
    L.bchk_tail_stats.argtypes = [vp, C.POINTER(u64)]
    L.bchk_coop_stats.argtypes = [vp, C.POINTER(u64)]
    L.bchk_tail_diag_read.argtypes = [vp, C.POINTER(u64), sz, C.POINTER(u64)]
    L.bchk_tail_prof_read.argtypes = [vp, C.POINTER(u64), sz]
    L.bchk_profile_read_stages.argtypes = [vp, C.POINTER(dbl), C.POINTER(u64)]
    L.bchk_set_analytic.argtypes = [vp, i32]
    L.bchk_set_chunk_limit.argtypes = [vp, C.c_uint32]
    L.bchk_kernel_ebch.argtypes = [i32, vp]
    L.bchk_kernel_field_order.argtypes = [i32, vp, vp]
    L.bchk_kernel_trellis_cost.argtypes = [vp, i32, vp, i32, C.POINTER(u64), C.POINTER(u64)]
    L.bchk_kernel_column_costs.argtypes = [i32, vp, vp, i32, vp, vp]
    L.bchk_kernel_column_search.argtypes = [i32, vp, vp, i32, u64, C.POINTER(u64), i32, vp, vp,
                                            C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_int64)]
    L.bchk_kernel_bec_masks.argtypes = [vp, i32, vp, sz, i32, vp]
    L.bchk_kernel_bec_behaviour.argtypes = [vp, i32, i32, i32, i32, vp]
    L.bchk_kernel_bec_sample.argtypes = [vp, i32, u64, u64, i32, vp, vp, vp, i32, vp]
    L.bchk_kernel_bec_capacity.argtypes = [vp, i32, i32, dbl, C.POINTER(dbl)]
    L.bchk_kernel_write_file.argtypes = [C.c_char_p, vp, i32, vp]
    L.bchk_polar_design_bec.argtypes = [C.c_char_p, C.c_char_p, i32, dbl, u64, u64, i32, vp, C.c_char_p, sz,
                                        C.POINTER(sz)]
    L.bchk_polar_genie_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp]
    L.bchk_polar_genie_run.argtypes = [vp, dbl, u64, u64, u64, sz, vp, vp, C.POINTER(dbl)]
    L.bchk_polar_design_genie.argtypes = [C.c_char_p, C.c_char_p, i32, dbl, u64, u64, i32, vp, vp, C.c_char_p, sz,
                                          C.POINTER(sz)]
    L.bchk_polar_generate_channel_device.argtypes = [vp, i32, dbl, sz, u64, u64, vp, vp, vp, vp, vp, vp]
    L.bchk_polar_sweep_channel_device.argtypes = [vp, i32, dbl, dbl, i32, u64, u64, u64, sz, vp, C.POINTER(dbl),
                                                  C.POINTER(u64)]
    L.bchk_polar_genie_run_channel.argtypes = [vp, i32, dbl, u64, u64, u64, sz, vp, vp, C.POINTER(dbl)]
    L.bchk_polar_design_genie_channel.argtypes = [C.c_char_p, C.c_char_p, i32, i32, dbl, u64, u64, i32, vp, vp,
                                                  C.c_char_p, sz, C.POINTER(sz)]
    L.bchk_polar_create_q8.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.POINTER(vp)]
    L.bchk_polar_create_q8_tiered.argtypes = [C.c_char_p, C.c_char_p, i32, i32, i32, C.POINTER(vp)]
    L.bchk_polar_decode_q8_host.argtypes = [vp, vp, sz, vp, vp, vp, vp]
    L.bchk_polar_decode_q8_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp]
    L.bchk_polar_quantize_device.argtypes = [vp, vp, sz, C.c_float, i32, vp, vp]
    L.bchk_polar_sweep_q8_device.argtypes = [vp, i32, dbl, dbl, i32, u64, u64, u64, sz, vp, C.POINTER(dbl),
                                             C.POINTER(u64), C.c_float, i32]
    L.bchk_polar_generate_fading_device.argtypes = [vp, i32, dbl, dbl, sz, u64, u64, vp, vp, vp, vp, vp, vp]
    L.bchk_polar_sweep_fading_device.argtypes = [vp, i32, dbl, dbl, dbl, i32, u64, u64, u64, sz, vp, C.POINTER(dbl),
                                                 C.POINTER(u64)]
    L.bchk_polar_sweep_q8_fading_device.argtypes = [vp, i32, dbl, dbl, dbl, i32, u64, u64, u64, sz, vp, C.POINTER(dbl),
                                                    C.POINTER(u64), C.c_float, i32]
    L.bchk_polar_genie_run_fading.argtypes = [vp, i32, dbl, dbl, u64, u64, u64, sz, vp, vp, C.POINTER(dbl)]
    L.bchk_polar_design_genie_fading.argtypes = [C.c_char_p, C.c_char_p, i32, i32, dbl, dbl, u64, u64, i32, vp, vp,
                                                 C.c_char_p, sz, C.POINTER(sz)]
    L.bchk_last_error.restype = C.c_char_p
    L.bchk_version.restype = C.c_char_p
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise BchkError(f"bchk error {rc}: {lib().bchk_last_error().decode()}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class FadingChannel:
    """A fading model with a parameter, for channel= wherever a channel name is taken:
    FadingChannel("rayleigh_block", S) (block size S, an integer >= 1), ("rayleigh_correlated", rho)
    (0 <= rho < 1) or ("rician", K) (K-factor, finite and >= 0). snr_db of the call is the average
    Eb/N0; include/bchk.h (BCHK_FADING_*) states the models."""

    def __init__(self, kind, param):
        if not isinstance(kind, str) or kind not in FADINGS:
            raise ValueError(f"kind must be one of {sorted(FADINGS)}, not {kind!r}")
        if isinstance(param, bool) or not isinstance(param, numbers.Real):  # no strings, no truth values
            raise ValueError(f"{kind}: the parameter must be a real number, not {param!r}")
        value = float(param)
        if kind == "rayleigh_block" and not (math.isfinite(value) and value >= 1.0 and value == math.floor(value)):
            raise ValueError(f"rayleigh_block: the block size must be an integer >= 1, not {param!r}")
        if kind == "rayleigh_correlated" and not 0.0 <= value < 1.0:
            raise ValueError(f"rayleigh_correlated: rho must lie in [0, 1), not {param!r}")
        if kind == "rician" and not 0.0 <= value < float("inf"):
            raise ValueError(f"rician: the K-factor must be finite and >= 0, not {param!r}")
        self.kind, self.param = kind, value

    def __repr__(self):
        return f"FadingChannel({self.kind!r}, {self.param!r})"


def _channel(channel):
    """BCHK_CHANNEL_* of "awgn" | "rayleigh" | "bsc"; a FadingChannel gives its (BCHK_FADING_*, param)."""
    if isinstance(channel, FadingChannel):
        return FADINGS[channel.kind], channel.param
    try:
        return CHANNELS[channel]
    except (KeyError, TypeError):
        raise ValueError(f"channel must be one of {sorted(CHANNELS)}, not {channel!r}") from None


class KanekoKernelProcessor:
    """Batched KanekoKernelProcessor (headers/KanekoKernelProcessor.h:47-68) for one
    BCH(n, k) code with t = designed correction capability, on one gfx950 device."""

    def __init__(self, m, t, J=BCHK_J_SHIPPED, decoder_snr_db=0.5, device=0):
        L = lib()
        h = C.c_void_p()
        _check(L.bchk_create(m, t, J, decoder_snr_db, device, C.byref(h)))
        self._h = h
        n, k, gs = C.c_int(), C.c_int(), C.c_int()
        _check(L.bchk_code_params(h, C.byref(n), C.byref(k), C.byref(gs)))
        self.m, self.t, self.J = m, t, J
        self.n, self.k = n.value, k.value
        self.g = np.zeros(gs.value, np.uint8)
        _check(L.bchk_generator(h, _p(self.g)))

    def close(self):
        if getattr(self, "_h", None):
            lib().bchk_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the module globals may already be gone: the process
        # teardown releases the device memory then
        try:
            self.close()
        except (TypeError, AttributeError):
            pass

    @property
    def handle(self):
        return self._h

    def set_max_decodes(self, md):
        _check(lib().bchk_set_max_decodes(self._h, int(md)))

    def decode(self, y, res=None, variant=VARIANT_ANSWER):
        """y [B, n] f64 -> (res [B, n] u8, l0 [B] f64, stats [B] STATS_DTYPE).
        Rows that are never accepted keep the incoming `res` content (default 0)."""
        y = np.ascontiguousarray(np.atleast_2d(y), np.float64)
        B = y.shape[0]
        assert y.shape[1] == self.n
        res = np.zeros((B, self.n), np.uint8) if res is None else np.ascontiguousarray(res, np.uint8)
        l0 = np.zeros(B, np.float64)
        st = np.zeros(B, STATS_DTYPE)
        _check(lib().bchk_decode_variant_host(self._h, variant, _p(y), B, _p(res), _p(l0), _p(st)))
        return res, l0, st

    def decode_device(self, d_y, B, d_res, d_l0, d_st, stream=None):
        _check(lib().bchk_decode_device(self._h, C.c_void_p(d_y), B, C.c_void_p(d_res),
                                        C.c_void_p(d_l0), C.c_void_p(d_st),
                                        C.c_void_p(stream) if stream else None))

    def count_device(self, d_tx, d_res, d_st, B, d_out6, stream=None):
        _check(lib().bchk_count_device(self._h, C.c_void_p(d_tx), C.c_void_p(d_res),
                                       C.c_void_p(d_st), B, C.c_void_p(d_out6),
                                       C.c_void_p(stream) if stream else None))

    def decode_count_device(self, d_y, d_tx, B, d_res, d_l0, d_st, d_out6, stream=None):
        """decode_device + count_device fused (bchk_decode_count_device); d_st may be 0."""
        _check(lib().bchk_decode_count_device(self._h, C.c_void_p(d_y), C.c_void_p(d_tx), B, C.c_void_p(d_res),
                                              C.c_void_p(d_l0), C.c_void_p(d_st) if d_st else None,
                                              C.c_void_p(d_out6), C.c_void_p(stream) if stream else None))

    def alg_decode(self, words, syndromes=None):
        """Decoder::decode batch: words [N, n] u8 -> (ok [N] bool, answers [N, n] u8)."""
        words = np.ascontiguousarray(np.atleast_2d(words), np.uint8)
        N = words.shape[0]
        ans = np.zeros_like(words)
        ok = np.zeros(N, np.uint8)
        sp = None
        if syndromes is not None:
            syndromes = np.ascontiguousarray(syndromes, np.uint32)
            sp = _p(syndromes)
        _check(lib().bchk_alg_decode_host(self._h, _p(words), sp, N, _p(ans), _p(ok)))
        return ok.astype(bool), ans

    def generate(self, snr_db, B, seed=1, state=0):
        """The reference input stream: (tx [B, n] u8, y [B, n] f64, next_state)."""
        tx = np.zeros((B, self.n), np.uint8)
        y = np.zeros((B, self.n), np.float64)
        st = C.c_uint64(state)
        _check(lib().bchk_generate_host(self._h, snr_db, B, C.byref(st), seed, _p(tx), _p(y)))
        return tx, y, st.value

    def generate_draws(self, snr_db, B, seed=1, state=0):
        """generate() and the engine draws it consumed: (tx, y, next_state, draws)."""
        tx = np.zeros((B, self.n), np.uint8)
        y = np.zeros((B, self.n), np.float64)
        st, dr = C.c_uint64(state), C.c_uint64()
        _check(lib().bchk_generate_host_draws(self._h, snr_db, B, C.byref(st), seed, _p(tx), _p(y),
                                              C.byref(dr)))
        return tx, y, st.value, dr.value

    def sweep_block(self, snr_db, state, skip, B):
        """One block of a sharded fun() sweep (bchk_sweep_block): (tx, res, accepted,
        ops [B, 3] = decodes/comparisons/sums, states [B] after each word, state after)."""
        tx = np.zeros((B, self.n), np.uint8)
        res = np.zeros((B, self.n), np.uint8)
        acc = np.zeros(B, np.uint8)
        ops = np.zeros((B, 3), np.uint64)
        states = np.zeros(B, np.uint64)
        st = C.c_uint64(state)
        _check(lib().bchk_sweep_block(self._h, snr_db, C.byref(st), skip, B, _p(tx), _p(res), _p(acc),
                                      _p(ops), _p(states)))
        return tx, res, acc, ops, states, st.value

    def sweep_range(self, snr_db, state, draws, max_words):
        """The words of `draws` engine draws from word start `state` (bchk_sweep_range), as
        sweep_block: (tx, res, accepted, ops, states, state after)."""
        tx = np.zeros((max_words, self.n), np.uint8)
        res = np.zeros((max_words, self.n), np.uint8)
        acc = np.zeros(max_words, np.uint8)
        ops = np.zeros((max_words, 3), np.uint64)
        states = np.zeros(max_words, np.uint64)
        st, nw = C.c_uint64(state), C.c_size_t()
        _check(lib().bchk_sweep_range(self._h, snr_db, C.byref(st), draws, max_words, _p(tx), _p(res), _p(acc),
                                      _p(ops), _p(states), C.byref(nw)))
        B = nw.value
        return tx[:B], res[:B], acc[:B], ops[:B], states[:B], st.value

    def sweep(self, p, e, max_snr=5.0, seed=1, batch=0, state=0, return_state=False):
        """fun() on the GPU: the reference CSV text (and the engine state after it)."""
        buf = C.create_string_buffer(1 << 16)
        st = C.c_uint64(state)
        _check(lib().bchk_sweep(self._h, p, e, max_snr, C.byref(st), seed, batch, buf, len(buf)))
        return (buf.value.decode(), st.value) if return_state else buf.value.decode()

    def generate_device(self, snr, B, d_tx, d_y, seed=1, word0=0, stream=None):
        """On-GPU channel: words [word0, word0 + B) of the counter-based stream into d_tx, d_y."""
        _check(lib().bchk_generate_device(self._h, snr, B, seed, word0, C.c_void_p(d_tx), C.c_void_p(d_y),
                                          C.c_void_p(stream) if stream else None))

    def sweep_device(self, p, e, max_snr=5.0, seed=1, batch=0):
        """fun() with GPU-generated words: (CSV text, seconds, words decoded)."""
        buf = C.create_string_buffer(1 << 16)
        secs, words = C.c_double(0.0), C.c_uint64(0)
        _check(lib().bchk_sweep_device(self._h, p, e, max_snr, seed, batch, buf, len(buf), C.byref(secs),
                                       C.byref(words)))
        return buf.value.decode(), secs.value, words.value

    def sync(self):
        _check(lib().bchk_sync(self._h))

    @property
    def stream(self):
        return lib().bchk_stream(self._h)

    def profile(self, enable=True):
        _check(lib().bchk_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        """([fast, exact, coop] kernel ms summed, decode calls) since the last read."""
        ms = (C.c_double * 3)()
        n = C.c_uint64()
        _check(lib().bchk_profile_read(self._h, ms, C.byref(n)))
        return list(ms), n.value

    def profile_read_stages(self):
        """([fast, exact first pass, coop, analytic tail] kernel ms, decode calls)."""
        ms = (C.c_double * 4)()
        n = C.c_uint64()
        _check(lib().bchk_profile_read_stages(self._h, ms, C.byref(n)))
        return list(ms), n.value

    def tail_count(self):
        """Codewords the last call's first pass handed to the analytic tail kernel."""
        a = C.c_uint64()
        _check(lib().bchk_tail_count(self._h, C.byref(a)))
        return a.value

    def tail_stats(self):
        """Last call's analytic tail outcomes: [handed on, finished, split, split chunks,
        enumeration steps, max steps per codeword]."""
        a = (C.c_uint64 * 6)()
        _check(lib().bchk_tail_stats(self._h, a))
        return list(a)

    def coop_stats(self):
        """Last call's cooperative-kernel counters (m >= 7): [dense re-decodes served,
        heavy codewords started]."""
        a = (C.c_uint64 * 2)()
        _check(lib().bchk_coop_stats(self._h, a))
        return list(a)

    def tail_diag(self, items=65536):
        """Diagnostics (context created with BCHK_TAIL_DIAG=1): per-codeword tail records."""
        import numpy as np
        out = np.zeros((items, 8), np.uint64)
        n = C.c_uint64()
        _check(lib().bchk_tail_diag_read(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), items,
                                         C.byref(n)))
        return out[:min(items, n.value)]

    def tail_prof(self, items=65536):
        """Experiment builds (BCHK_AN_PROF): enumeration cycles by step phase per tail record."""
        import numpy as np
        out = np.zeros((items, 8), np.uint64)
        _check(lib().bchk_tail_prof_read(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), items))
        return out

    def set_analytic(self, enable=True):
        """Analytic tail of heavy codewords (results identical either way)."""
        _check(lib().bchk_set_analytic(self._h, 1 if enable else 0))

    def set_chunk_limit(self, chunks):
        """64-pattern chunks of the exact first pass before the tail / hand-off."""
        _check(lib().bchk_set_chunk_limit(self._h, int(chunks)))

    def path_counts(self):
        """(codewords handed to the exact kernel, to the cooperative kernel) last call."""
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().bchk_path_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_fast_path(self, enable=True):
        _check(lib().bchk_set_fast_path(self._h, 1 if enable else 0))

    def set_syndrome_table(self, enable=True):
        """Syndrome decoding table of the search kernels (results identical either way)."""
        _check(lib().bchk_set_syndrome_table(self._h, 1 if enable else 0))

    def first_pass_waves(self):
        """Resident waves of the first exact pass (its queue items below that are not claimed)."""
        w = C.c_uint32()
        _check(lib().bchk_first_pass_waves(self._h, C.byref(w)))
        return w.value


class PolarListDecoder:
    """CMixedKernelListDecoder(Spec, ListSize) + Decode (out/external/MixedKernelListDecoder.cpp
    :9, :211-268) on the GPU: batched SC-list decoding of a polar code given by the
    reference's specification text, and the BPSK simulation around it over AWGN, Rayleigh fading
    and the BSC (encode_device, generate_device, count_device, sweep_device:
    out/external/Simulator.cpp). Layers: "A"
    (Arikan), matrix files ("-file"), and the library's named kernels "G" (3 x 3) and "A5"
    (5 x 5, rows as CA5Kernel::Multiply computes them), in any case, decoded by their own f/g
    processors with the state carried per path: code lengths such as 12, 24, 40, 60, 96. With
    L > 1 the lists are the reference's bit for bit where the reference is defined (every G
    the innermost layer; A5 anywhere), see include/bchk.h and DESIGN 5.14.

    state="lds" keeps every path's state in LDS, which bounds the length (about U L <= 36000 for
    all-Arikan codes). state="tiered" (all-Arikan codes, U <= 16384, any L <= 32) moves the layers
    1..split to a device-memory workspace shared between the paths, with the same
    lists bit for bit; split=None lets the library choose the boundary. state="tiered_mixed" is
    that state for codes with matrix or named layers (and all-Arikan ones, through the same
    kernel, csrc/polar_mixed_tiered.hip): the state of the layers before `split`, counted from the
    channel side, lives in the workspace; codes with an ordered-statistics layer
    stay on state="lds".

    llr="q8" (all-Arikan codes) is the fixed-point decoder: decode and decode_device
    take int8 LLRs (quantize / quantize_device make them), the path state is a third of the f32
    one's, and sweep_device needs a scale. With state="lds" every path's state is in LDS (about
    U L <= 65536); state="tiered_q8" (U <= 16384, any L <= 32; llr="q8" only) is that decoder in
    the tiered state (csrc/polar_sclist_q8_tiered.hip): the layers 1..split in the
    workspace with the LLRs as bytes, the same lists bit for bit, split=None as for "tiered".
    llr="f32" is everything above."""

    llr = "f32"  # the instance's number format ("q8": the fixed-point decoder)

    def __init__(self, spec, L, device=0, kernel_dir=None, state="lds", split=None, llr="f32"):
        if state not in ("lds", "tiered", "tiered_mixed", "tiered_q8"):
            raise ValueError(f"state must be 'lds', 'tiered', 'tiered_mixed' or 'tiered_q8', not {state!r}")
        if state == "lds" and split is not None:
            raise ValueError("split applies to the tiered states only")
        if llr not in ("f32", "q8"):
            raise ValueError(f"llr must be 'f32' or 'q8', not {llr!r}")
        if llr == "q8" and state not in ("lds", "tiered_q8"):
            raise ValueError("llr='q8' takes state='lds' or, for the tiered state, state='tiered_q8'")
        if state == "tiered_q8" and llr != "q8":
            raise ValueError("state='tiered_q8' is the fixed-point decoder: llr must be 'q8'")
        self.llr = llr
        h = C.c_void_p()
        kdir = kernel_dir.encode() if kernel_dir else None
        if state == "tiered_q8":
            _check(lib().bchk_polar_create_q8_tiered(spec.encode(), kdir, L, device, -1 if split is None else int(split),
                                                     C.byref(h)))
        elif llr == "q8":
            _check(lib().bchk_polar_create_q8(spec.encode(), kdir, L, device, C.byref(h)))
        elif state != "lds":
            create = lib().bchk_polar_create_tiered if state == "tiered" else lib().bchk_polar_create_tiered_mixed
            _check(create(spec.encode(), kdir, L, device, -1 if split is None else int(split), C.byref(h)))
        else:
            _check(lib().bchk_polar_create_kdir(spec.encode(), kdir, L, device, C.byref(h)))
        self._h = h
        n, k, u, l = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _check(lib().bchk_polar_params(h, C.byref(n), C.byref(k), C.byref(u), C.byref(l)))
        self.N, self.K, self.U, self.L = n.value, k.value, u.value, l.value

    def close(self):
        if getattr(self, "_h", None):
            lib().bchk_polar_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib().bchk_polar_stream(self._h)

    def state_info(self):
        """dict(split, lds_bytes, workspace_bytes, grid): the boundary in use (0: all in LDS), LDS and
        workspace bytes per workgroup (one codeword in flight each), workgroups of a launch."""
        s, g, l, w = C.c_int(), C.c_int(), C.c_uint64(), C.c_uint64()
        _check(lib().bchk_polar_state_info(self._h, C.byref(s), C.byref(l), C.byref(w), C.byref(g)))
        return dict(split=s.value, lds_bytes=l.value, workspace_bytes=w.value, grid=g.value)

    @property
    def split(self):
        """The layers 1..split are in the device-memory tier (0: every layer in LDS)."""
        return self.state_info()["split"]

    def encode(self, info):
        info = np.ascontiguousarray(info, np.uint8)
        cw = np.zeros((info.shape[0], self.N), np.uint8)
        _check(lib().bchk_polar_encode_host(self._h, _p(info), info.shape[0], _p(cw)))
        return cw

    def decode(self, llr):
        """llr [B][N] float32 -> (count [B], info [B][L][K], codewords [B][L][N], metrics [B][L]).
        On a q8 decoder llr is int8 (an array of another type is refused, not converted)."""
        if self.llr == "q8":
            if np.asarray(llr).dtype != np.int8:
                raise TypeError("a q8 decoder takes int8 LLRs (see quantize)")
            llr = np.ascontiguousarray(llr, np.int8)
            call = lib().bchk_polar_decode_q8_host
        else:
            llr = np.ascontiguousarray(llr, np.float32)
            call = lib().bchk_polar_decode_host
        B = llr.shape[0]
        info = np.zeros((B, self.L, self.K), np.uint8)
        cw = np.zeros((B, self.L, self.N), np.uint8)
        met = np.zeros((B, self.L), np.float32)
        cnt = np.zeros(B, np.int32)
        _check(call(self._h, _p(llr), B, _p(info), _p(cw), _p(met), _p(cnt)))
        return cnt, info, cw, met

    def decode_device(self, d_llr, B, d_info, d_cw, d_metric, d_count, stream=None):
        """Device pointers; d_llr [B][N] is f32, or int8 on a q8 decoder."""
        call = lib().bchk_polar_decode_q8_device if self.llr == "q8" else lib().bchk_polar_decode_device
        _check(call(self._h, d_llr, B, d_info, d_cw, d_metric, d_count, stream))

    def quantize_device(self, d_llr, count, d_q, scale, qmax=63, stream=None):
        """d_q[i] = clamp(rint(d_llr[i] * scale), -qmax, qmax), i < count (device pointers, f32 ->
        int8): quantize() on the GPU, on any decoder."""
        _check(lib().bchk_polar_quantize_device(self._h, d_llr or None, count, scale, qmax, d_q or None, stream))

    def encode_device(self, d_info, B, d_cw, stream=None):
        """The encoder on the GPU: d_info [B][K] u8 -> d_cw [B][N] u8 (device pointers)."""
        _check(lib().bchk_polar_encode_device(self._h, d_info or None, B, d_cw or None, stream))

    def generate_device(self, snr_db, B, d_llr, d_info=None, d_cw=None, seed=1, word0=0, stream=None,
                        channel="awgn", d_h=None, d_y=None):
        """On-GPU channel: words [word0, word0 + B) of the counter-based stream at Eb/N0 snr_db into
        d_llr [B][N] f32 and, where given, d_info [B][K] and d_cw [B][N]. channel = "awgn",
        "rayleigh" (real Rayleigh fading known to the receiver, snr_db the average Eb/N0) or "bsc"
        (snr_db is then the crossover probability p, LLRs +-2); information bits and codewords do
        not depend on it. d_h and d_y [B][N] f64, where given, receive the fading factor (Rayleigh
        and the FadingChannel models) and the channel output. channel may also be a FadingChannel."""
        chan = _channel(channel)
        tail = (snr_db, B, seed, word0, d_info or None, d_cw or None, d_llr or None, d_h or None, d_y or None, stream)
        if isinstance(chan, tuple):
            _check(lib().bchk_polar_generate_fading_device(self._h, *chan, *tail))
        else:
            _check(lib().bchk_polar_generate_channel_device(self._h, chan, *tail))

    def count_device(self, d_info_tx, d_cw_tx, d_llr, d_info, d_cw, d_count, B, d_out8, d_flags=None,
                     stream=None):
        """The simulator's counters of one decoded batch added into d_out8 (device uint64[8],
        POLAR_COUNTERS); d_flags [B] u8 (optional): bit 0 block, 1 ML, 2 list error."""
        _check(lib().bchk_polar_count_device(self._h, d_info_tx or None, d_cw_tx or None, d_llr or None,
                                             d_info or None, d_cw or None, d_count or None, B, d_out8 or None,
                                             d_flags or None, stream))

    def sweep_device(self, snr_from, snr_step, points, max_words, max_errors, seed=1, batch=0, channel="awgn",
                     scale=None, qmax=63):
        """The FER simulation end to end on the GPU: ([(snr_db, counters [8] ints)], seconds,
        words decoded). Each point runs until max_words words or max_errors block errors, cut
        exactly in word order; the word index runs on across points. channel as for
        generate_device; on "bsc" the points are crossover probabilities. A q8 decoder needs
        `scale` (each batch is quantised with (scale, qmax) as by quantize_device before it is
        decoded); an f32 decoder refuses one."""
        chan = _channel(channel)
        if (scale is not None) != (self.llr == "q8"):
            raise ValueError("scale is required on a q8 decoder" if self.llr == "q8"
                             else "scale applies to a q8 decoder only")
        out = np.zeros(max(points, 0), POLAR_POINT_DTYPE)
        secs, words = C.c_double(0.0), C.c_uint64(0)
        fading = isinstance(chan, tuple)
        args = (self._h, *(chan if fading else (chan,)), snr_from, snr_step, points, max_words, max_errors, seed, batch,
                _p(out) if points > 0 else None, C.byref(secs), C.byref(words))
        L = lib()
        if self.llr == "q8":
            _check((L.bchk_polar_sweep_q8_fading_device if fading else L.bchk_polar_sweep_q8_device)(*args, scale, qmax))
        else:
            _check((L.bchk_polar_sweep_fading_device if fading else L.bchk_polar_sweep_channel_device)(*args))
        return [(float(r["snr_db"]), [int(v) for v in r["c"]]) for r in out], secs.value, words.value

    def genie_device(self, d_info_tx, d_llr, B, d_err, d_soft, d_dec_llr=None, d_u=None, stream=None):
        """Genie-aided SC of one batch (device pointers): symbol phi of every word decoded with the
        true earlier symbols fed back. d_err (u64) and d_soft (i64), [U] each, are added into (the
        definitions: include/bchk.h); d_dec_llr [B][U] f32 and d_u [B][U] u8, where given, receive
        the decision LLRs and the rebuilt encoder inputs."""
        _check(lib().bchk_polar_genie_device(self._h, d_info_tx or None, d_llr or None, B, d_err or None,
                                             d_soft or None, d_dec_llr or None, d_u or None, stream))

    def genie_run(self, snr_db, words, seed=1, word0=0, batch=0, channel="awgn"):
        """Words [word0, word0 + words) of generate_device's stream through genie_device:
        (err [U] u64, soft [U] i64, seconds), a function of (code, channel, snr_db, seed, word0,
        words). channel as for generate_device."""
        err = np.zeros(self.U, np.uint64)
        soft = np.zeros(self.U, np.int64)
        secs = C.c_double(0.0)
        chan = _channel(channel)
        tail = (snr_db, words, seed, word0, batch, _p(err), _p(soft), C.byref(secs))
        if isinstance(chan, tuple):
            _check(lib().bchk_polar_genie_run_fading(self._h, *chan, *tail))
        else:
            _check(lib().bchk_polar_genie_run_channel(self._h, chan, *tail))
        return err, soft, secs.value

    def sync(self):
        _check(lib().bchk_polar_sync(self._h))

    def last_launches(self):
        """Kernel launches the last decode call took (time-budgeted codes with search layers)."""
        n = C.c_uint64()
        _check(lib().bchk_polar_last_launches(self._h, C.byref(n)))
        return n.value

    def scratch_bytes(self):
        """(device scratch held for budgeted calls and the tiered workspace, bytes of one workgroup's
        save slot)."""
        b, s = C.c_uint64(), C.c_uint64()
        _check(lib().bchk_polar_scratch_bytes(self._h, C.byref(b), C.byref(s)))
        return b.value, s.value


def quantize(llr, scale, qmax=63):
    """The rule of PolarListDecoder.quantize_device in numpy: int8 clamp(rint(llr * scale), -qmax,
    qmax), the product formed in float32, ties to even, NaN -> 0, +-inf -> +-qmax."""
    if not 1 <= int(qmax) <= 127:
        raise ValueError(f"qmax = {qmax}: the int8 range is 1..127")
    if not 0.0 < float(np.float32(scale)) < np.inf:
        raise ValueError(f"scale = {scale} must be positive and finite")
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.asarray(llr, np.float32) * np.float32(scale))
    return np.clip(np.where(np.isnan(v), np.float32(0), v), -qmax, qmax).astype(np.int8)


def stream_skip(k, n, state, words):
    """(engine state, draws) after `words` stream words from `state` (no samples, no device)."""
    st, dr = C.c_uint64(), C.c_uint64()
    _check(lib().bchk_stream_skip(k, n, state, words, C.byref(st), C.byref(dr)))
    return st.value, dr.value


def stream_sync(k, n, state, offset, limit):
    """A word start in [offset, offset + limit) draws from word start `state` that depends only
    on (state, offset, limit) -- where every parse possible at `offset` has merged, not
    necessarily the first start at or after it -- found without parsing the draws before
    `offset`: (draws from state, engine state), or None when unresolved."""
    off, st = C.c_uint64(), C.c_uint64()
    rc = lib().bchk_stream_sync(k, n, state, offset, limit, C.byref(off), C.byref(st))
    if rc == 1:
        return None
    _check(rc)
    return off.value, st.value


def rng_jump(state, draws):
    """The reference engine's state `draws` draws after `state` (a seed is a state)."""
    return int(lib().bchk_rng_jump(int(state), int(draws)))


MINSTD_PERIOD = 2147483646  # minstd_rand0: 2^31 - 2


def syndrome_table_query(m, t, syndromes):
    """Host-side Decoder::decode through the syndrome table (no GPU): syndromes [N][t] odd
    syndromes S_1, S_3, ... as uint32 -> (ok [N] bool, flipped-position masks [N] uint64)."""
    syn = np.ascontiguousarray(syndromes, np.uint32)
    N = syn.shape[0]
    ok = np.zeros(N, np.uint8)
    err = np.zeros(N, np.uint64)
    _check(lib().bchk_syndrome_table_query(m, t, _p(syn), N, _p(ok), _p(err)))
    return ok.astype(bool), err


def syndrome_table_info(m, t):
    """(distinct keys, bytes, longest probe sequence) of the (m, t) syndrome table."""
    k, b, p = C.c_uint64(), C.c_uint64(), C.c_uint32()
    _check(lib().bchk_syndrome_table_info(m, t, C.byref(k), C.byref(b), C.byref(p)))
    return k.value, b.value, p.value


KERNEL_INFO_FIELDS = ("tmax", "fast", "lane", "selection", "table", "tail")


def kernel_info(m, t):
    """The kernels a context for (m, t) would launch (bchk_kernel_info, no GPU): a dict of
    KERNEL_INFO_FIELDS. BchkError where bchk_create refuses (m, t)."""
    out = (C.c_int32 * 8)()
    _check(lib().bchk_kernel_info(m, t, out))
    return dict(zip(KERNEL_INFO_FIELDS, (int(v) for v in out)))


def kernel_ebch(power):
    """makeMatrix (root bchCoder.cpp:356-389): the nested extended-BCH kernel, 2^power square."""
    n = 1 << power
    K = np.zeros((n, n), np.uint8)
    _check(lib().bchk_kernel_ebch(power, _p(K)))
    return K


def kernel_field_order(power, K):
    """swapColumns' column reordering (root bchCoder.cpp:478-496)."""
    K = np.ascontiguousarray(K, np.uint8)
    out = np.zeros_like(K)
    _check(lib().bchk_kernel_field_order(power, _p(K), _p(out)))
    return out


def kernel_trellis_cost(K, llr, device=0):
    """(SumCount, CmpCount) of CTrellisKernelProcessor::GetLLRs over every phase with zero known
    inputs (the column search's score), computed on the GPU."""
    K = np.ascontiguousarray(K, np.uint8)
    y = np.ascontiguousarray(llr, np.float32)
    s, c = C.c_uint64(), C.c_uint64()
    _check(lib().bchk_kernel_trellis_cost(_p(K), K.shape[0], _p(y), device, C.byref(s), C.byref(c)))
    return s.value, c.value


def kernel_column_costs(power, K, llr, device=0):
    """Scores of every L.U column map (indexed by candidate code), from one GPU launch."""
    K = np.ascontiguousarray(K, np.uint8)
    y = np.ascontiguousarray(llr, np.float32)
    n = 1 << (power * (power - 1))
    s = np.zeros(n, np.uint64)
    c = np.zeros(n, np.uint64)
    _check(lib().bchk_kernel_column_costs(power, _p(K), _p(y), device, _p(s), _p(c)))
    return s, c


KSEARCH_EXHAUSTIVE, KSEARCH_RANDOM = 0, 1


def kernel_column_search(power, K, llr, mode=KSEARCH_EXHAUSTIVE, count=0, rng_state=1, device=0):
    """randomSwapColumns (root bchCoder.cpp:541-699) -> dict(best, perm, sum, cmp, index,
    rng_state)."""
    K = np.ascontiguousarray(K, np.uint8)
    y = np.ascontiguousarray(llr, np.float32)
    n = 1 << power
    best = np.zeros((n, n), np.uint8)
    perm = np.zeros(n, np.uint32)
    st, s, c, i = C.c_uint64(rng_state), C.c_uint64(), C.c_uint64(), C.c_int64()
    _check(lib().bchk_kernel_column_search(power, _p(K), _p(y), mode, count, C.byref(st), device,
                                           _p(best), _p(perm), C.byref(s), C.byref(c), C.byref(i)))
    return dict(best=best, perm=perm, sum=s.value, cmp=c.value, index=i.value, rng_state=st.value)


def kernel_bec_masks(K, patterns, device=0):
    """Per erasure pattern (uint64, bit j = column j erased) the mask of uncorrectable phases
    (bit i = phase i) of the invertible kernel K (2 <= l <= 64), computed on the GPU."""
    K = np.ascontiguousarray(K, np.uint8)
    pat = np.ascontiguousarray(patterns, np.uint64)
    masks = np.zeros(pat.shape[0], np.uint64)
    _check(lib().bchk_kernel_bec_masks(_p(K), K.shape[0], _p(pat), pat.shape[0], device, _p(masks)))
    return masks


def kernel_bec_behaviour(K, w_lo=0, w_hi=None, device=0):
    """Exact BEC polarisation behaviour of K (l <= 32): counts [l][l + 1] uint64, counts[i][w] =
    the weight-w erasure patterns that leave phase i uncorrectable, for w_lo <= w <= w_hi
    (default: every weight), enumerated on the GPU."""
    K = np.ascontiguousarray(K, np.uint8)
    l = K.shape[0]
    counts = np.zeros((l, l + 1), np.uint64)
    _check(lib().bchk_kernel_bec_behaviour(_p(K), l, w_lo, l if w_hi is None else w_hi, device, _p(counts)))
    return counts


def kernel_bec_sample(K, samples, seed=1, device=0, pattern_weight=None):
    """The same for l <= 64 with at most `samples` patterns per weight -> (unc [l][l + 1], tried
    [l + 1], exact [l + 1] bool): weights with C(l, w) <= samples enumerated, the others sampled
    from the Philox stream `seed`; counts[i][w] is estimated by unc C(l, w) / tried. With
    pattern_weight, also the patterns tried at that weight (uint64)."""
    K = np.ascontiguousarray(K, np.uint8)
    l = K.shape[0]
    unc = np.zeros((l, l + 1), np.uint64)
    tried = np.zeros(l + 1, np.uint64)
    exact = np.zeros(l + 1, np.uint8)
    pat = None if pattern_weight is None else np.zeros(samples, np.uint64)
    _check(lib().bchk_kernel_bec_sample(_p(K), l, samples, seed, device, _p(unc), _p(tried), _p(exact),
                                        0 if pat is None else pattern_weight, None if pat is None else _p(pat)))
    if pat is None:
        return unc, tried, exact.astype(bool)
    return unc, tried, exact.astype(bool), pat[:int(tried[pattern_weight])]


def kernel_bec_capacity(counts, phase, capacity):
    """CBECCapacityEvaluator::GetSubchannelCapacity: the capacity of `phase` of the kernel with
    BEC table counts [l][l + 1] over a BEC of the given capacity (host only)."""
    counts = np.ascontiguousarray(counts, np.uint64)
    out = C.c_double()
    _check(lib().bchk_kernel_bec_capacity(_p(counts), counts.shape[0], phase, capacity, C.byref(out)))
    return out.value


def write_kernel_file(path, K, counts=None):
    """A kernel file in the reference's format: size, matrix and, with counts [l][l + 1], the BEC
    section (channel id 3) its capacity evaluator parses."""
    K = np.ascontiguousarray(K, np.uint8)
    if counts is not None:
        counts = np.ascontiguousarray(counts, np.uint64)
        if counts.shape != (K.shape[0], K.shape[0] + 1):
            raise BchkError("counts must be [l][l + 1]")
    _check(lib().bchk_kernel_write_file(os.fsencode(path), _p(K), K.shape[0], None if counts is None else _p(counts)))


def design_bec(layers, K, capacity=0.5, kernel_dir=None, samples=1 << 16, seed=1, device=0):
    """BEC design of a polar code over the kernels of `layers` (names, or the spec's layer line):
    -> (spec text for PolarListDecoder, capacities [U] of the symbols). Matrix kernels take
    their BEC table from their file, or from the GPU when the file has none. The named
    kernels "G" / "A5" are refused (BchkError naming the kernel): use design_genie."""
    line = layers if isinstance(layers, str) else " ".join(layers)
    cap = np.zeros(16384, np.float64)
    buf = C.create_string_buffer(64 + len(line) + 8 * 16384)
    needed = C.c_size_t()
    _check(lib().bchk_polar_design_bec(line.encode(), kernel_dir.encode() if kernel_dir else None, K, capacity,
                                       samples, seed, device, _p(cap), buf, len(buf), C.byref(needed)))
    spec = buf.value.decode()
    return spec, cap[:int(spec.split()[0])].copy()


def design_genie(layers, K, snr_db, words, kernel_dir=None, seed=1, device=0, channel="awgn"):
    """Monte-Carlo design over the kernels of `layers`: the symbols ranked by their genie-aided
    error counts over `words` words of the stream `seed` at Eb/N0 snr_db (ties: the larger soft sum,
    then the higher index) -> (spec text for PolarListDecoder, err [U] u64, soft [U] i64).
    Layers may be "A", matrix files, and the named kernels "G" and "A5". channel = "awgn",
    "rayleigh", "bsc" (snr_db is then the crossover probability) or a FadingChannel: the design is
    for that channel."""
    line = layers if isinstance(layers, str) else " ".join(layers)
    err = np.zeros(16384, np.uint64)
    soft = np.zeros(16384, np.int64)
    buf = C.create_string_buffer(64 + len(line) + 8 * 16384)
    needed = C.c_size_t()
    chan = _channel(channel)
    head = (line.encode(), kernel_dir.encode() if kernel_dir else None, K)
    tail = (snr_db, words, seed, device, _p(err), _p(soft), buf, len(buf), C.byref(needed))
    if isinstance(chan, tuple):
        _check(lib().bchk_polar_design_genie_fading(*head, *chan, *tail))
    else:
        _check(lib().bchk_polar_design_genie_channel(*head, chan, *tail))
    spec = buf.value.decode()
    U = int(spec.split()[0])
    return spec, err[:U].copy(), soft[:U].copy()


def version():
    return lib().bchk_version().decode()

from . import sweep_dist  # noqa: E402,F401  (sharded fun() sweep over ranks)
