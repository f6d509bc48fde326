"""bbb_awgn_hist's way through the host scheduler under the stream / event model of tests/sched_model/ (see
tests/test_sched_model.py): the REAL bbb_api.hip and the REAL hist_api.hip compiled for the host, the histogram kernels
replaced by stubs that record what they read and write, and random sequences that mix histograms with fills, announcements,
staging levels, the noise stream object and a re-bound caller stream (tests/sched_model/hist_driver.cpp).

lutopt_stage_visit runs the produce half every staged call runs (staged_produce in bbb_api.hip) with the caller's kernel in the
mover's place.  It must come through clean, and two mutants must be FOUND: the slot's "free" event no longer standing for a
reader on the caller's other stream (the mover_chain rule of test_sched_model.py, here with the histogram mover as that
reader), and a staged call that claims to be independent of the previous sample kernel when its start states were not
announced (its in-line seeding then overwrites start states that kernel still reads).  The second removes the independence
decision of the SHARED path -- staged_produce's `int rc = begin_op(h, true, h->pf.matches(seed_step, L, G));`, the line every staged fill,
transmitter call and stage visit goes through -- so here it is found on a stage visit or on a fill, whichever comes first."""
import json
import subprocess

import pytest

from conftest import ROOT

CSRC = ROOT / "basebandboard_amd" / "csrc"
MODEL = ROOT / "tests" / "sched_model"
TAPS = str(ROOT / "basebandboard_amd" / "data" / "lutopt_256.taps")

MUTANTS = {
    "mover_chain": [("""    if ((rc = sl.wait_free(ms))) return rc;
""", "")],
    "visit_independent": [("int rc = begin_op(h, true, h->pf.matches(seed_step, L, G));", "int rc = begin_op(h, true, true);")],
}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched_model_hist")
    api = (CSRC / "bbb_api.hip").read_text()
    common = ["-std=c++17", "-O1", "-g", "-I", str(MODEL), "-I", str(CSRC)]
    rest = ["-x", "c++", str(CSRC / "hist_api.hip"), "-x", "none", str(MODEL / "model.cpp"), str(MODEL / "detector_stub.cpp"), str(MODEL / "hist_driver.cpp"), "-ldl", "-lpthread"]
    procs = {}
    cmd = ["g++", *common, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-x", "c++", str(CSRC / "bbb_api.hip"), *rest, "-o", str(d / "asan")]
    procs["asan"] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, edits in MUTANTS.items():
        text = api
        for old, new in edits:
            assert text.count(old) == 1, f"mutant {name}: its rule occurs {text.count(old)} times in bbb_api.hip (expected once)"
            text = text.replace(old, new)
        src = d / f"bbb_api_{name}.cpp"
        src.write_text(text)
        procs[name] = subprocess.Popen(["g++", *common, str(src), *rest, "-o", str(d / name)], stdout=subprocess.PIPE,
                                       stderr=subprocess.PIPE, text=True)
    for name, pr in procs.items():
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (name, err[-4000:])
    return {name: d / name for name in procs}


def run(exe, nseq, seed, max_bad=1000000):
    r = subprocess.run([str(exe), TAPS, str(nseq), str(seed), str(max_bad)], capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def test_histograms_among_other_calls_order_every_access(exes):
    for seed, nseq in ((1, 2500), (2, 1500)):
        r, out = run(exes["asan"], nseq, seed)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        assert out["sequences_with_unordered_access"] == 0 and out["sequences"] == nseq
        assert out["histograms"] > 3 * nseq and out["operations_checked"] > 20 * nseq


@pytest.mark.parametrize("mutant,what", [("mover_chain", "hist_planes_kernel"), ("visit_independent", "seed")])
def test_the_model_sees_the_histogram_path(exes, mutant, what):
    r, out = run(exes[mutant], 4000, 1, max_bad=3)
    assert r.returncode == 1 and out["sequences_with_unordered_access"] > 0
    assert "UNORDERED ACCESS" in r.stderr and what in r.stderr
