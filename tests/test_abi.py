"""The C-ABI library loads, exports every symbol include/bbb.h declares, and its host-only entry
points behave (no compute call is made: there is no GPU here and no CPU compute path)."""
import ctypes as C
import re

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT
from oracle import jump


def header_symbols():
    text = (ROOT / "include" / "bbb.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(bbb_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported():
    lib = _lib.lib()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), s
    assert sorted(_lib.SYMBOLS) == syms
    assert lib.bbb_abi_version() == 1


def test_no_torch_types_or_oracle_in_product():
    """The boundary is plain C; the product never touches the oracle."""
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "bbb.h").read_text(), flags=re.S)
    assert "torch" not in hdr and "at::" not in hdr and "Tensor" not in hdr
    for p in (ROOT / "basebandboard_amd").rglob("*"):
        if p.suffix in (".py", ".hip", ".hpp", ".cpp", ".inc"):
            assert "oracle" not in p.read_text().lower(), p


def test_strerror_and_invalid_arguments():
    lib = _lib.lib()
    assert lib.bbb_strerror(0) == b"ok"
    assert b"invalid" in lib.bbb_strerror(_lib.BBB_EINVAL)
    s = C.c_uint64()
    assert lib.bbb_prbs_state_at(8, 1, 10, C.byref(s)) == _lib.BBB_EINVAL
    assert b"k=8 invalid for PRBS" in lib.bbb_last_error_detail()
    assert lib.bbb_prbs_fill(12, 1, 0, 64, None, 0, None) == _lib.BBB_EINVAL
    assert lib.bbb_prbs_detector_run(10, None, 1, 1, None, None, 0, None) == _lib.BBB_EINVAL
    with pytest.raises(ValueError, match="k=10 invalid for PRBS"):
        bbb.PRBS(10)
    with pytest.raises(ValueError, match="k=10 invalid for PRBS"):
        bbb.PRBSErrorDetector(10)
    assert sorted(bbb.TAPS) == [7, 9, 11, 15, 20, 23, 31]


def test_compute_without_gpu_fails_loudly():
    """No device here: compute entry points must return BBB_ENODEV, never compute on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _lib.lib()
    assert lib.bbb_prbs_fill(31, 1, 0, 64, C.c_void_p(16), 0, None) == _lib.BBB_ENODEV
    with pytest.raises(_lib.BbbError) as e:
        bbb.LUTOPT.shipped(256)
    assert e.value.code == _lib.BBB_ENODEV
    u = bbb.LUTOPT.shipped(256, device=-1)            # host-only handle: algebra works, compute refuses
    assert lib.bbb_awgn_fill_i8(u._h, C.c_void_p(16), 16, 0) == _lib.BBB_ENODEV
    cfg = _lib.TrialCfg(31, 10, 1, 0, 1, 16, 0, 100)
    out = _lib.Ber()
    assert lib.bbb_ber_trials(u._h, C.byref(cfg), 1, C.byref(out)) == _lib.BBB_ENODEV


@pytest.mark.parametrize("k", (7, 9, 11, 15, 20, 23, 31))
def test_prbs_jump_ahead_host(oracle, k):
    """bbb_prbs_state_at (GF(2) jump) against the sequential oracle."""
    p = bbb.PRBS(k)
    for n in (0, 1, 5, 64, 1000, 123_457):
        assert p.state_at(n) == oracle.prbs_bits(k, n)[1]
    a, b = 10**12 + 7, 98_765
    mid = bbb.PRBS(k, init=p.state_at(a))
    assert mid.state_at(b) == p.state_at(a + b) == jump.prbs_state(k, 1, a + b)      # composition alone is blind to a jump error that commutes
    assert p.state_at((1 << k) - 1) == 1               # maximal length: period 2^k - 1


@pytest.mark.parametrize("n", (16, 32, 64, 128, 256, 512))
def test_lutopt_jump_ahead_host(oracle, golden_lutopt, n):
    """bbb_lutopt_state_at on a host-only handle against the oracle and the golden states."""
    u = bbb.LUTOPT.shipped(n, device=-1)
    m = oracle.Lutopt(path=oracle.data_path(n))
    if str(n) in golden_lutopt:
        for i, h in enumerate(golden_lutopt[str(n)]["states_hex"][:20]):
            assert u.state_at(i + 1) == int(h, 16)
    for t in (0, 1, 2, 63, 64, 1000, 20_011):
        assert u.state_at(t) == m.run_int(1, t)
    init = (0x0123456789ABCDEF << (n - 64 if n > 64 else 0) | 5) & ((1 << n) - 1)
    v = bbb.LUTOPT.shipped(n, init=init, device=-1)
    assert v.state_at(3333) == m.run_int(init, 3333)
    far = bbb.LUTOPT.shipped(n, init=v.state_at(10**17), device=-1)
    assert far.state_at(4242) == v.state_at(10**17 + 4242) == jump.lutopt_state(m, init, 10**17 + 4242)     # (tests/test_jump_host.py)
    assert u.specialised == (n == 256)


def test_matrix_file_loader(tmp_path):
    # the reference's 0/1 text format (software/rnghunt/matrices/N), as rnghunt.rs:51-53 writes it
    ref_fmt = tmp_path / "32"
    ref_fmt.write_text("".join("".join("1" if c in row else "0" for c in range(32)) + "\n" for row in bbb.recurrences.n32))
    u = bbb.LUTOPT.from_matrix_file(ref_fmt, device=-1)
    assert u.packed == bbb.recurrences.n32 and u.k == 32
    assert bbb.recurrences.load_packed(ref_fmt) == bbb.recurrences.n32
    assert np.array_equal(u.a.sum(axis=1), [len(r) for r in bbb.recurrences.n32])
    bad = tmp_path / "bad.txt"
    bad.write_text("010\n10\n001\n")
    with pytest.raises(_lib.BbbError) as e:
        bbb.LUTOPT.from_matrix_file(bad, device=-1)
    assert e.value.code == _lib.BBB_EIO
    with pytest.raises(_lib.BbbError):
        bbb.LUTOPT.from_matrix_file(tmp_path / "missing.txt", device=-1)
    with pytest.raises(ValueError):
        bbb.LUTOPT.from_packed([[0, 30]] * 24, device=-1)            # tap index out of range
    with pytest.raises(ValueError):
        bbb.LUTOPT.from_packed([[0, 0]] * 24, device=-1)             # duplicate tap in a row
    assert bbb.LUTOPT.from_packed([[0, 1]] * 24, device=-1).k == 24   # LUTOPT itself accepts any k (rng.py:21-40)


def test_shipped_matrices_have_lut_friendly_weights():
    """Row and column weights 3..4 (what the LUT-optimised search produces: rnghunt.rs:25)."""
    for n in bbb.recurrences.SIZES:
        p = bbb.recurrences.load_packed(bbb.recurrences.matrix_path(n))
        assert len(p) == n and set(map(len, p)) <= {3, 4}
        col = np.zeros(n, dtype=int)
        for r in p:
            col[r] += 1
        assert set(col.tolist()) <= {3, 4}


def test_channel_helpers():
    from basebandboard_amd import channel
    assert channel.amp_for_ebn0(0.0, 8) == 91             # 64 * sqrt(2) = 90.5
    assert abs(channel.ebn0_db(91, 8) - 0.0) < 0.05
    assert abs(channel.ber_theory(0.0) - 0.0786) < 1e-3
    assert channel.shard(10, 1, 4) == [1, 5, 9]
    with pytest.raises(ValueError, match="invalid for PRBS"):
        bbb.Trial(10, 1, 1, prbs_k=12)


def test_header_is_plain_c(tmp_path):
    """include/bbb.h must be usable from C (the cgo / JNI / FFI side of a host): C11, no C++ constructs."""
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "bbb.h"\nint main(void) { bbb_trial_cfg c; bbb_detector_stats s; (void)c; (void)s; return BBB_OK; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", f"-I{ROOT / 'include'}", str(src)])


def test_cpp_caller_links_against_the_library():
    """examples/bbb_mc.cpp: a plain C++ program on the C ABI (built by build()); it must link and, without a
    GPU, fail with the library's own error rather than run anything on the CPU."""
    import subprocess
    exe = ROOT / "examples" / "bbb_mc"
    if not exe.exists():
        subprocess.check_call(["make", "-C", str(ROOT / "examples")])
    import torch
    if torch.cuda.is_available():
        pytest.skip("covered by the GPU test")
    r = subprocess.run([str(exe), "--bits", "1000"], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and ("no usable" in r.stderr.lower() or "device" in r.stderr.lower() or "hip" in r.stderr.lower())


def test_product_sources_carry_no_experiment_code_and_the_overlays_apply(tmp_path):
    """Round 5: the laboratory's instrumentation (per-wave time stamps, suppressed stores, extra kernel arguments) lives in
    experiments/overlays/<file>.json and is applied to COPIES of the product sources when libbbb_hip_exp.so is built
    (tools/exp_overlay.py, csrc/Makefile).  The product sources contain no `#if ... BBB_EXPERIMENTS` block and no test-only revert
    macro -- the one place the macro is defined for is env_knob() in bbb_common.hpp, which is a constant in the product -- and every
    overlay still finds its place (a product edit that touches instrumented lines must take its overlay along)."""
    import subprocess
    import sys
    csrc = ROOT / "basebandboard_amd" / "csrc"
    for f in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.hpp")):
        text = f.read_text()
        assert "BBB_SCHED_MODEL" not in text, f.name
        if f.name == "bbb_common.hpp":
            continue
        assert not re.search(r"^\s*#\s*if.*BBB_EXPERIMENTS", text, re.M), f.name
    overlays = sorted((ROOT / "experiments" / "overlays").glob("*.json"))
    assert {o.name for o in overlays} >= {"awgn_kernels.hip.json", "ber_kernels_impl.hpp.json", "prbs_kernels.hip.json"}
    for o in overlays:
        src = csrc / o.name[:-len(".json")]
        out = tmp_path / src.name
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "exp_overlay.py"), "apply", str(src), str(o), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, (o.name, r.stdout + r.stderr)
        assert "BBB_EXPERIMENTS" in out.read_text() and len(out.read_text()) > len(src.read_text())
