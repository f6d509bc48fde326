"""The stream detector's host scheduler -- basebandboard_amd/csrc/detector_api.hip, UNCHANGED: det_plan, the pooled workspace,
the lease a call holds on a slot, the first pass in its four forms, the verify pass, the repairs queued blind and after a look,
the general repair loop and the serial continuation -- under the stream / event model of tests/sched_model/ (see
tests/test_sched_model.py).  The launchers of detector_launch.hpp are stubs that record what the real kernels read and write and
every scalar they are given; tests/sched_model/detector_driver.cpp plays two caller streams that own their buffers and makes
random sequences of calls over every k, lengths from one word to several thousand chunks, explicit and default geometries,
an input off its 16-byte boundary, with and without outputs and statistics, refused calls and calls that fail at a launch --
so that a slot is reused by a call with another layout on the other stream.  The model has no values, so the driver scripts what
every read-back delivers and holds the statistics that come back to what its script implies.

The transcript says what was queued: a refactor of detector_api.hip must leave it as it was (build the driver against the file
before the change and after it, same seeds).  No value is pinned here; what is held is that every access is ordered, under
AddressSanitizer + UndefinedBehaviorSanitizer (leaks included: the pool is immortal but reachable), that the statistics are the
script's, that every form and every outcome of the verify pass occurred, that the transcript is a function of the seed alone,
that det_plan agrees with tests/detector_geometry.py, and that the model sees the two rules the workspace's reuse rests on."""
import json
import subprocess

import pytest

from conftest import ROOT
from detector_geometry import KS, default_chunk_words, form_of
from test_gpu_detector_forms import FUSED, K20_ONLY, TWO_KERNEL

CSRC = ROOT / "basebandboard_amd" / "csrc"
MODEL = ROOT / "tests" / "sched_model"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]

# MUTANTS: detector_api.hip with ONE ordering rule taken out of a copy, by exact text that must occur exactly once
# (test_sched_model.py's rule)
MUTANTS = {
    # a call that finds the previous user's zeroing of the tail pending waits for it: without the wait a call with another
    # layout on the other stream writes its chunk records while that memset may still run
    "no_zero_wait": ("        if (zero_pending) (void)hipStreamWaitEvent(st, w->ev_zero, 0);\n", ""),
    # the lease's destructor synchronises the call's stream before the slot goes back: without it a call that returned early
    # (a failing launch) leaves work in flight on a slot the next call takes
    "no_lease_sync": ("        if (!leave_zeroed) (void)hipStreamSynchronize(st);\n", ""),
}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sched_model_detector")
    rest = [str(MODEL / "model.cpp"), str(MODEL / "detector_driver.cpp"), "-ldl", "-lpthread"]
    inc = ["-I", str(MODEL), "-I", str(CSRC)]
    cmds = {"driver": ["g++", "-std=c++17", "-O1", "-g", *SAN, *inc, "-x", "c++", str(CSRC / "detector_api.hip"), "-x", "none", *rest,
                       "-o", str(d / "driver")]}
    text = (CSRC / "detector_api.hip").read_text()
    for name, (old, new) in MUTANTS.items():
        assert text.count(old) == 1, f"mutant {name}: its rule occurs {text.count(old)} times in detector_api.hip (expected once)"
        src = d / f"detector_api_{name}.cpp"
        src.write_text(text.replace(old, new))
        cmds[name] = ["g++", "-std=c++17", "-O1", "-g", *inc, str(src), *rest, "-o", str(d / name)]
    procs = {name: subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for name, cmd in cmds.items()}
    for name, pr in procs.items():
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (name, err[-4000:])
    return {name: d / name for name in procs}


def run(exe, nseq, seed, max_bad=1000000):
    r = subprocess.run([str(exe), str(nseq), str(seed), str(max_bad)], capture_output=True, text=True, timeout=900,
                       env={"ASAN_OPTIONS": "detect_leaks=1"})
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def test_the_detector_scheduler_orders_every_access(exes):
    """Two seeds.  The driver itself ends with an error when a call's statistics -- chunks, chunks_rerun, serial_fallback and the
    four totals from the right half of the tail -- are not what the scripted read-backs imply, or when a scripted read-back was
    not read; LeakSanitizer reports what is not reachable at exit (the pool's slots are: it is allocated with new and kept)."""
    for seed, nseq in ((1, 1500), (2, 1000)):
        r, out = run(exes["driver"], nseq, seed)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        assert "LeakSanitizer" not in r.stderr and "runtime error" not in r.stderr
        assert out["sequences_with_unordered_access"] == 0 and out["sequences"] == nseq
        assert out["calls"] > 5 * nseq and out["operations_checked"] > 50 * nseq
        # every form of the first pass, every outcome of the verify pass, refused and failing calls, and slots reused with
        # another layout on the other stream
        assert all(n > nseq // 10 for n in out["forms"].values()), out["forms"]
        assert set(out["outcomes"]) == {"consistent_sparse", "consistent_dense", "repaired_sparse", "repaired_dense", "many_bad",
                                        "second_verify_bad", "serial"}
        assert all(n > nseq // 20 for n in out["outcomes"].values()), out["outcomes"]
        assert out["refused"] > nseq // 10 and out["failed_launches"] > nseq // 10 and out["other_layout_other_stream"] > nseq // 2


def test_transcript_is_a_function_of_the_seed_alone(exes):
    r1, a = run(exes["driver"], 200, 5)
    r2, b = run(exes["driver"], 200, 5)
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-3000:], r2.stderr[-3000:])
    assert len(a["transcript"]) == 16 and a["transcript"] == b["transcript"]
    _, other = run(exes["driver"], 200, 6)
    assert other["transcript"] != a["transcript"]


@pytest.mark.parametrize("mutant,what", [("no_zero_wait", "memset"), ("no_lease_sync", "det_")])
def test_the_model_finds_a_slot_reused_too_early(exes, mutant, what):
    """The workspace is reused by the next call, on whichever stream: it must come after the zeroing the previous call left
    queued behind its read-back, and after everything a call that returned early had queued."""
    r, out = run(exes[mutant], 1000, 1, max_bad=3)
    assert r.returncode == 1 and out["sequences_with_unordered_access"] > 0
    assert "UNORDERED ACCESS" in r.stderr and what in r.stderr


# test_detector_geometry_host.py::test_default_geometry_at_the_lengths_in_use
LENGTHS = (300_001, 2_000_000, 1_000_000_000, 2_120_000_000, 2_147_000_000, 4_260_000_000, 8_590_000_000, 10_000_000_000)


def test_det_plan_agrees_with_the_restatement(exes):
    """det_plan's form and chunk length against detector_geometry.form_of / default_chunk_words: every k, the chunk / warm-up
    pairs of test_gpu_detector_forms.py and the default geometry, at the lengths in use, on and off a 16-byte boundary."""
    asked = []
    for k in KS:
        for nbits in LENGTHS:
            for al in (0, 8):
                for cw, wb in FUSED + TWO_KERNEL + K20_ONLY:
                    asked.append(((k, nbits, cw * 64, wb, al, 256), (form_of(k, cw, wb, aligned16=al == 0), cw)))
                for ncu in (256, 304, 64):
                    words = default_chunk_words(nbits, ncu)
                    asked.append(((k, nbits, 0, 0, al, ncu), (form_of(k, words, 1024, aligned16=al == 0), words)))
    text = "".join(" ".join(str(v) for v in a) + "\n" for a, _ in asked)
    r = subprocess.run([str(exes["driver"]), "plan"], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(got) == len(asked)
    for (a, (form, words)), g in zip(asked, got):
        assert (g["k"], g["nbits"], g["chunk_bits"], g["warm_bits"], g["alignment"], g["ncu"]) == a
        assert (g["form"], g["chunk_words"]) == (form, words), (a, g)
