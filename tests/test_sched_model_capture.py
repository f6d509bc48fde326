"""The capture side -- the three objects that own a device and a stream (bbb_errstat, bbb_nco, bbb_sinc_eye) and the stateless
calls that take samples or packed bits the caller already holds (bbb_eye_accumulate_i16, bbb_acf_accumulate_i16,
bbb_xcorr_accumulate_i16, bbb_fir_filter / _slice, bbb_ddc_run, bbb_sinc_interpolate, bbb_prbs_check, bbb_shaper_fill_i16,
bbb_awgn_hist) -- under the stream / event model of tests/sched_model/ (see tests/test_sched_model.py): the REAL bbb_api.hip,
errstat_api.hip, nco_api.hip, sinc_api.hip, eye_api.hip, acf_api.hip, xcorr_api.hip, fir_api.hip, ddc_api.hip and hist_api.hip
(with capture.hpp, what they share) compiled for the host, their kernels replaced by stubs that record what they read and write
and every scalar argument, and random sequences over two caller streams that open the objects with random settings, run them
across their chunk and launch bounds, re-bind their streams (also to the one they are on), read, set and reset their state,
close them with work still queued, and make the stateless and refused calls between (tests/sched_model/capture_driver.cpp).

The transcript says what was queued and what was refused, with which text: a refactor of these host files must leave it as it
was (build the driver against the csrc/ before the change and after it, same seeds).  No value is pinned here; what is held is
that every access is ordered, under AddressSanitizer + UndefinedBehaviorSanitizer (leaks included), that the transcript is a
function of the seed alone, and that the model sees a re-bound stream that does not wait for the old one."""
import json
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "basebandboard_amd" / "csrc"
MODEL = ROOT / "tests" / "sched_model"
TAPS = str(ROOT / "basebandboard_amd" / "data" / "lutopt_256.taps")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
API = ["bbb_api.hip", "errstat_api.hip", "nco_api.hip", "sinc_api.hip", "eye_api.hip", "acf_api.hip", "xcorr_api.hip", "fir_api.hip",
       "ddc_api.hip", "hist_api.hip"]

# the MUTANT: capture.hpp's StreamObj::rebind with its wait taken out, by exact text (test_sched_model.py's rule: the text must
# occur exactly once)
REBIND = "capture.hpp"
WAIT = ("if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);\n", "")


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched_model_capture")
    # the mutant's files are copies in a directory of their own, so that every file that includes the header finds the copy
    mut = d / "mut"
    mut.mkdir()
    for f in list(CSRC.glob("*.hpp")) + [CSRC / a for a in API]:
        shutil.copy(f, mut / f.name)
    text = (CSRC / REBIND).read_text()
    assert text.count(WAIT[0]) == 1, f"the wait of the stream re-binding occurs {text.count(WAIT[0])} times in {REBIND} (expected once)"
    (mut / REBIND).write_text(text.replace(*WAIT))
    rest = ["-x", "none", str(MODEL / "model.cpp"), str(MODEL / "detector_stub.cpp"), str(MODEL / "capture_driver.cpp"), "-ldl", "-lpthread"]
    cmds = {
        "driver": ["g++", "-std=c++17", "-O1", "-g", *SAN, "-I", str(MODEL), "-I", str(CSRC), "-x", "c++", *[str(CSRC / a) for a in API],
                   *rest, "-o", str(d / "driver")],
        # (-I csrc: bbb_common.hpp's relative path to include/bbb.h is found from there)
        "no_wait": ["g++", "-std=c++17", "-O1", "-g", "-I", str(MODEL), "-I", str(mut), "-I", str(CSRC), "-x", "c++",
                    *[str(mut / a) for a in API], *rest, "-o", str(d / "no_wait")],
    }
    procs = {name: subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for name, cmd in cmds.items()}
    for name, pr in procs.items():
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (name, err[-4000:])
    return {name: d / name for name in procs}


def run(exe, nseq, seed, max_bad=1000000):
    r = subprocess.run([str(exe), TAPS, str(nseq), str(seed), str(max_bad)], capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def test_the_capture_side_orders_every_access(exes):
    for seed, nseq in ((1, 1500), (2, 1000)):
        r, out = run(exes["driver"], nseq, seed)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        assert out["sequences_with_unordered_access"] == 0 and out["sequences"] == nseq
        assert out["calls"] > 15 * nseq and out["operations_checked"] > 50 * nseq
        # runs across a chunk or launch bound, and refused calls, in most sequences
        assert out["chunked"] > nseq // 2 and out["refused"] > nseq // 2


def test_transcript_is_a_function_of_the_seed_alone(exes):
    r1, a = run(exes["driver"], 200, 5)
    r2, b = run(exes["driver"], 200, 5)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-3000:], r2.stderr[-3000:])
    assert len(a["transcript"]) == 16 and a["transcript"] == b["transcript"]
    _, other = run(exes["driver"], 200, 6)
    assert other["transcript"] != a["transcript"]


def test_the_model_finds_a_rebound_stream_that_does_not_wait(exes):
    """An object re-bound to the caller's other stream without the wait: what it queues there reads and writes the object's
    state while the launches on the old stream may still do so."""
    r, out = run(exes["no_wait"], 1000, 1, max_bad=3)
    assert r.returncode == 1 and out["sequences_with_unordered_access"] > 0
    assert "UNORDERED ACCESS" in r.stderr and ("nco_" in r.stderr or "errstat_" in r.stderr)
