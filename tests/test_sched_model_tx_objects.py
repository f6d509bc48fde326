"""The five objects that walk the transmitter's waveform chunk by chunk -- bbb_tx_eye, bbb_tx_ber_sweep, bbb_tx_acf,
bbb_link_sweep, bbb_tx_xcorr -- under the stream / event model of tests/sched_model/ (see tests/test_sched_model.py): the REAL
bbb_api.hip and the REAL eye_api.hip, txsweep_api.hip, acf_api.hip, link_api.hip, xcorr_api.hip (with tx_chunks.hpp, the loop
they share) compiled for the host, their kernels replaced by stubs that record what they read and write and every scalar
argument, and random sequences that open each object with random settings (noise on or off, PRBS or Pulser, small chunks),
run ranges of 1, 2 and more chunks with a ragged last one from sample 0 and elsewhere among plain fills, and close them
(tests/sched_model/tx_objects_driver.cpp).

The transcript says what the objects queued: a refactor of these host files must leave it as it was (build the driver against
the csrc/ before the change and after it, same seeds).  No value is pinned here; what is held is that every access is ordered,
under AddressSanitizer + UndefinedBehaviorSanitizer (leaks included), and that the transcript is a function of the seed alone.
tests/sched_model/tx_bits_check.cpp, under the same sanitizers, holds the four bit-range functions to the buffers the opens size."""
import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "basebandboard_amd" / "csrc"
MODEL = ROOT / "tests" / "sched_model"
TAPS = str(ROOT / "basebandboard_amd" / "data" / "lutopt_256.taps")
SAN = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-I", str(MODEL), "-I", str(CSRC)]
API = ["bbb_api.hip", "eye_api.hip", "txsweep_api.hip", "acf_api.hip", "link_api.hip", "xcorr_api.hip", "fir_api.hip"]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched_model_tx_objects")
    cmds = {
        "driver": ["g++", *SAN, "-x", "c++", *[str(CSRC / f) for f in API], "-x", "none", str(MODEL / "model.cpp"),
                   str(MODEL / "detector_stub.cpp"), str(MODEL / "tx_objects_driver.cpp"), "-o", str(d / "driver"), "-ldl", "-lpthread"],
        "bits": ["g++", *SAN, str(MODEL / "tx_bits_check.cpp"), "-o", str(d / "bits")],
    }
    procs = {name: subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for name, cmd in cmds.items()}
    for name, pr in procs.items():
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (name, err[-4000:])
    return {name: d / name for name in procs}


def run(exe, nseq, seed):
    r = subprocess.run([str(exe), TAPS, str(nseq), str(seed)], capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def test_the_objects_among_other_calls_order_every_access(exes):
    for seed, nseq in ((1, 1500), (2, 1000)):
        r, out = run(exes["driver"], nseq, seed)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        assert out["sequences_with_unordered_access"] == 0 and out["sequences"] == nseq
        assert out["runs"] > 4 * nseq and out["operations_checked"] > 100 * nseq


def test_transcript_is_a_function_of_the_seed_alone(exes):
    r1, a = run(exes["driver"], 200, 5)
    r2, b = run(exes["driver"], 200, 5)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-3000:], r2.stderr[-3000:])
    assert len(a["transcript"]) == 16 and a["transcript"] == b["transcript"]
    _, other = run(exes["driver"], 200, 6)
    assert other["transcript"] != a["transcript"]


def test_every_chunks_data_bits_fit_the_buffer_the_open_sizes(exes):
    r = subprocess.run([str(exes["bits"])], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-2000:], r.stderr[-4000:])
