"""The library's host scheduler -- basebandboard_amd/csrc/bbb_api.hip, UNCHANGED: staging slots, slot generations, the
prefetch swap, look-ahead, the stream objects, the transmitter's bit buffers, BER trials and continued trials -- compiled
for the host against a model of HIP streams and events (tests/sched_model/) and driven with random call sequences.  Every
kernel launch is replaced by a stub that records which device buffers the real kernel reads and writes; the model keeps
vector clocks and reports every access that the streams, events and host synchronisations do not order: a write in front
of a buffer's last reader, a read in front of its writer.  That is the hazard the GPU cannot be sanitised for and that
round 3's soak test met on seed 3 of 3.

Five MUTANTS prove that the model sees what it has to: copies of the file with ONE ordering rule removed by exact text (the
product source carries no test macro since round 5) -- round 3's race (an announcement that was never taken leaves its seeding
on one arithmetic stream, the next seeding goes to the other), the round-2 advisor's case (a prefetch's "the seeding waited for
this slot's mover" outliving later movers on the slot), round 4's rule that a slot's "free" event stands for ALL movers that read
it, round 5's turn-taking of the BER trials' generator buffers and of the transmitter's data-bit buffers -- all must be FOUND; the scheduler as it stands must come
through >= 10 000 sequences clean, under AddressSanitizer + UndefinedBehaviorSanitizer (leaks included) and under ThreadSanitizer."""
import json
import subprocess

import pytest

from conftest import ROOT

SRC = [str(ROOT / "tests" / "sched_model" / "model.cpp"), str(ROOT / "tests" / "sched_model" / "detector_stub.cpp"),
       str(ROOT / "tests" / "sched_model" / "driver.cpp")]
TAPS = str(ROOT / "basebandboard_amd" / "data" / "lutopt_256.taps")


BUILDS = {
    "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
    "tsan": ["-fsanitize=thread"],
}

# MUTANTS: the scheduler with ONE of its ordering rules taken out.  Until round 4 these were #ifdef holes in the product source
# (BBB_SCHED_MODEL_REVERT_*); now the product file carries no test macro and the rule is removed from a COPY of it, by exact text:
# every (old, new) pair must match exactly once -- a rule that is reworded in bbb_api.hip fails the test until its mutant follows.
MUTANTS = {
    # round 3's race (commit f1ee557's scheduler in that respect): an announcement that was never taken leaves its seeding on one
    # arithmetic stream, the next seeding goes to the other
    # (the event itself is created by its first record, as every ordering event is: only the wait goes)
    "untaken_hint": [("""    if (pf.seeded) BBB_HIP(hipStreamWaitEvent(side, pf.seeded, 0));
""", "")],
    # the round-2 advisor's case: a prefetch's "the seeding waited for this slot's mover" outliving later movers on the slot
    "stale_skip": [("h->pf_waited_slot == slot && h->pf_waited_gen == sl.gen;", "h->pf_waited_slot == slot;")],
    # round 4: a slot's "free" event stands for ALL movers that read it, also one on the caller's other stream
    # (StageSlot::wait_free at the mover's call site alone: the arithmetic stream's and the seeding's waits stay)
    "mover_chain": [("""    if ((rc = sl.wait_free(ms))) return rc;
""", "")],
    # round 5: a BER trial's generator buffers are taken in turn; the seeding of trial s + 2 must wait for the kernel of trial s
    "ber_buffer_reuse": [("""            if ((rc = gs.set.wait_read(ss))) return rc;    // the trial before last read this set
""", "")],
    # round 5: the transmitter's data bits take the staging slot's two bit buffers in turn INSTEAD of waiting for the slot's last mover;
    # without the turn the bits of the slot's next kernel are written while that mover still reads them
    "tx_bits_turn": [("bits_buf = sl.bits_turn ^= 1u;", "bits_buf = 0;")],
}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """the two sanitizer builds of the file as it is and one plain build per mutant, compiled side by side"""
    d = tmp_path_factory.mktemp("sched_model")
    api = (ROOT / "basebandboard_amd" / "csrc" / "bbb_api.hip").read_text()
    csrc = str(ROOT / "basebandboard_amd" / "csrc")
    procs = {}
    for name, flags in BUILDS.items():
        cmd = ["g++", "-std=c++17", "-O1", "-g", *flags, "-I", str(ROOT / "tests" / "sched_model"), "-x", "c++",
               str(ROOT / "basebandboard_amd" / "csrc" / "bbb_api.hip"), "-x", "none", *SRC, "-o", str(d / name), "-ldl", "-lpthread"]
        procs[name] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, edits in MUTANTS.items():
        text = api
        for old, new in edits:
            assert text.count(old) == 1, f"mutant {name}: its rule occurs {text.count(old)} times in bbb_api.hip (expected once)"
            text = text.replace(old, new)
        # (the copy lives elsewhere: its quoted includes are found through -I csrc)
        src = d / f"bbb_api_{name}.cpp"
        src.write_text(text)
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-I", str(ROOT / "tests" / "sched_model"), "-I", csrc, str(src), *SRC, "-o", str(d / name), "-ldl", "-lpthread"]
        procs[name] = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    for name, pr in procs.items():
        _, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (name, err[-4000:])
    return {name: d / name for name in procs}


def run(exe, nseq, seed, mode="all", max_bad=1000000, timeout=900):
    r = subprocess.run([str(exe), TAPS, str(nseq), str(seed), mode, str(max_bad)], capture_output=True, text=True, timeout=timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def test_scheduler_orders_every_access_over_ten_thousand_sequences(exes):
    exe = exes["asan"]
    total = 0
    for seed, nseq, mode in ((1, 7000, "all"), (2, 4000, "hints")):
        r, out = run(exe, nseq, seed, mode)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
        assert out["sequences_with_unordered_access"] == 0 and out["sequences"] == nseq and out["operations_checked"] > 10 * nseq
        total += out["sequences"]
    assert total >= 10_000


def test_scheduler_under_thread_sanitizer(exes):
    exe = exes["tsan"]
    r, out = run(exe, 1500, 3)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert out["sequences_with_unordered_access"] == 0 and "ThreadSanitizer" not in r.stderr


def test_transcript_is_the_same_for_the_same_seed_and_for_both_builds(exes):
    """The model's transcript -- a hash over every operation, wait, record, synchronisation, free and query answer it logs, with
    buffers, events and streams named by creation number -- says WHAT the scheduler queued: a refactor of bbb_api.hip must leave it
    as it was (compare a build against the file before the change with one against the file after it, same seeds).  No value is
    pinned here: a deliberate scheduler change alters it.  What is held is that it is a function of the call sequence alone."""
    r1, a = run(exes["asan"], 300, 5)
    r2, b = run(exes["asan"], 300, 5)
    r3, c = run(exes["tsan"], 300, 5)
    assert r1.returncode == 0 and r2.returncode == 0 and r3.returncode == 0, (r1.stderr[-3000:], r3.stderr[-3000:])
    assert len(a["transcript"]) == 16 and a["transcript"] == b["transcript"] == c["transcript"]
    _, other = run(exes["asan"], 300, 6)
    assert other["transcript"] != a["transcript"]


@pytest.mark.parametrize("macro,mode,what", [
    ("untaken_hint", "all", "seeding"),
    ("untaken_hint", "hints", "seeding"),
    ("stale_skip", "hints", "awgn256_planes_kernel"),
    ("mover_chain", "all", "awgn256_planes_kernel"),
    ("ber_buffer_reuse", "all", "seed_"),
    ("tx_bits_turn", "all", "memset"),
])
def test_the_model_finds_the_races_of_rounds_two_and_three(exes, macro, mode, what):
    """The scheduler with one of its ordering rules taken out: the model must report unordered accesses, and of the kind the
    rule is about (two seedings writing the same start-state buffers from different streams; a sample kernel overwriting a
    staging slot its mover still reads -- rounds 2 and 3; round 4, the mover on the caller's stream: a sample kernel
    overwriting a slot that a mover on the caller's OTHER stream still reads after a re-bind the caller did not order)."""
    r, out = run(exes[macro], 6000 if macro == "mover_chain" else 3000, 1, mode, max_bad=3)
    assert r.returncode == 1 and out["sequences_with_unordered_access"] > 0
    assert "UNORDERED ACCESS" in r.stderr and what in r.stderr


def test_model_reports_the_use_of_a_destroyed_stream(tmp_path):
    """Round 4's crash was not an ordering fault but a LIFETIME fault: a process-wide cache remembered a hipStream_t and
    synchronised with it after its owner had destroyed it.  The model's streams now carry a lifetime -- hipStreamDestroy poisons
    the handle, every later use is a report -- and tests/sched_model/lifetime_check.cpp holds it to that bug's shape: the
    stream-remembering cache must be reported on every kind of use, the event-based one that replaced it must not."""
    exe = tmp_path / "lifetime_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", str(ROOT / "tests" / "sched_model"), str(ROOT / "tests" / "sched_model" / "model.cpp"),
                        str(ROOT / "tests" / "sched_model" / "lifetime_check.cpp"), "-o", str(exe), "-ldl", "-lpthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok lifetimes"), (out.stdout + out.stderr)[-3000:]


def test_a_call_that_fails_at_a_launch_gives_its_timing_events_back(tmp_path):
    """The model's launches never fail, so the random sequences cannot see what a call that returns EARLY leaves behind.  With
    profiling on, tests/sched_model/leak_check.cpp makes a staged fill, an unstaged fill of the specialised kernel and a staged
    transmitter fill fail at each of their launches in turn (model::fail_nth_launch), checks that the call returns the error and
    destroys the handle: under AddressSanitizer's leak check every timing event the call had created must have found an owner.
    (Built against bbb_api.hip as it stood before its events were owned, the same program reports leaked events: profiles/README.md.)"""
    exe = tmp_path / "leak_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-I", str(ROOT / "tests" / "sched_model"), "-x", "c++",
                        str(ROOT / "basebandboard_amd" / "csrc" / "bbb_api.hip"), "-x", "none",
                        str(ROOT / "tests" / "sched_model" / "model.cpp"), str(ROOT / "tests" / "sched_model" / "detector_stub.cpp"),
                        str(ROOT / "tests" / "sched_model" / "leak_check.cpp"),
                        "-o", str(exe), "-ldl", "-lpthread"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe), TAPS], capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=1"})
    assert out.returncode == 0 and out.stdout.strip().endswith("ok no event outlives its call"), (out.stdout + out.stderr)[-3000:]
    assert "LeakSanitizer" not in out.stderr
