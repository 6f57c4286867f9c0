"""csrc/multi.hip at 1, 2, 3, 4 and 8 devices on a simulated node, on the CPU.

multi.hip is host code over the HIP runtime, RCCL and the public C ABI; it is
compiled UNCHANGED with the host compiler and linked with tests/cpp/multi_sim.cpp,
which defines all 34 symbols it needs: deferred streams, HIP's event binding,
fused p2p groups, five kinds of schedule, a hazard check, fake contexts,
release accounting and fault injection (the program's header describes them).
No pool machine has more than one GPU, so this is the only place where the
cross-device sends, the peers' "slot free again" events and receive offsets
for U > S run at all.

The mutants prove that the simulator can fail: one textual substitution each
in a copy of multi.hip, which must match exactly once, and the program must
then exit non-zero with a message of the expected kind.  Nothing of them is
kept.  Two of them are the same program at n = 1 and must pass there.

The two "slot free again" mutants are caught as hazards, not as wrong bytes,
and cannot be caught otherwise through the public interface.  Collecting step
k (sift_multi_gathered) waits on gdone[slot][0], which completes the whole
fused group of that gather, before the caller can enqueue step k + 2, the next
writer of the slot.  So a gather whose slot is overwritten early is always one
the caller skipped, and what it left in rk is replaced by the next gather on
the same stream.  The node therefore fails a run in which an op runs while a
conflicting op the host enqueued earlier is still pending, and the driver has a
pass that collects only after the flush.  These two mutants validate that
hazard check; they do not reach the byte comparison.

Built with the address and undefined-behaviour sanitizers (their runtimes linked
statically into the program) where the host compiler has them -- decided by an
empty program, so that a sanitizer build of the real one that fails is a
failure and not a quiet plain build -- and without them otherwise."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT

SIM = os.path.join(ROOT, "tests", "cpp", "multi_sim.cpp")
MULTI = os.path.join(ROOT, "sift-gpu_amd", "csrc", "multi.hip")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
BASE = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
        "-I", os.path.join(ROOT, "include"), "-I", ROCM_INCLUDE]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]

# name: (text in multi.hip, its replacement, the message the program must print,
#        True if the mutant is the original program at n = 1)
MUTANTS = {
    # compute of step k + 2 no longer waits until the gather of step k has read the slot
    "compute_skips_gdone_wait": (
        "      MHIP(m, hipStreamWaitEvent(cs, m->gdone[s][i], 0));  // step k - 2's gather has read slot s\n",
        "",
        r"hazard: detect #\d+ on compute stream .* ran while the earlier-enqueued (copy|p2p group)", False),
    # only device 0 marks its slot free again: the peers wait on the record made at creation
    "gdone_recorded_on_device_0_only": (
        "    MHIP(m, hipEventRecord(m->gdone[p][i], m->gstream[i]));\n",
        "    if (i == 0) MHIP(m, hipEventRecord(m->gdone[p][i], m->gstream[i]));\n",
        r"hazard: detect #\d+ on compute stream .* ran while the earlier-enqueued p2p group", True),
    # device 0 posts its record receives from itself
    "recv_peer_is_0": (
        "ncclUint8, i, m->comm[0], m->gstream[0]);",
        "ncclUint8, 0, m->comm[0], m->gstream[0]);",
        r"unpaired p2p op: rank 0 posts 0 sends to rank 0, which posts \d+ receives from it", True),
    # the descriptor receive lands at the record index, not at 128 floats per record
    "desc_recv_offset_unscaled": (
        "r = ncclRecv(m->rd + at * SIFT_DESC_LEN,",
        "r = ncclRecv(m->rd + at,",
        r"wrong bytes: descriptor \d+ of \d+ of gathered step", False),
    # the caller is handed rk before the gather that fills it has run
    "gathered_skips_gdone_wait": (
        "  MHIP(m, hipEventSynchronize(m->gdone[slot][0]));\n",
        "  (void)slot;\n",
        r"wrong bytes: record \d+ of \d+ of gathered step", False),
    # sub-batch j takes mask j, not the mask of its first image
    "mask_slice_by_sub_batch_index": (
        "d_masks[i] + (size_t)first * mask_img_stride",
        "d_masks[i] + (size_t)j * mask_img_stride",
        r"wrong slice: unit \d+ step \d+ \(first image \d+\) got the mask pointer", False),
    # a send or receive that fails inside the gather's group no longer closes the group:
    # reached only by the fault sweep, in a gather that crosses devices
    "failed_group_left_open": (
        "        (void)ncclGroupEnd();\n",
        "",
        r"call \d+ failed and left a p2p group open", False),
}


def _run(cmd):
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def toolchain(tmp_path_factory):
    """The simulator's object file and the flags every program here is built
    with: the sanitizer flags if the unchanged program builds with them."""
    d = tmp_path_factory.mktemp("multi_sim")
    obj, mobj, exe = str(d / "multi_sim.o"), str(d / "multi.o"), str(d / "multi_sim")

    def build(flags):
        with ThreadPoolExecutor(max_workers=2) as pool:
            objs = list(pool.map(_run, (BASE + flags + ["-c", SIM, "-o", obj],
                                        BASE + flags + ["-c", "-x", "c++", MULTI, "-o", mobj])))
        for r in objs + [_run(BASE + flags + [obj, mobj, "-o", exe])]:
            if r.returncode != 0:
                return r
        return None

    # the compiler has the sanitizers and their static runtimes iff an empty program builds with them
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = SAN if _run(["g++"] + SAN + [str(probe), "-o", str(d / "probe")]).returncode == 0 else []
    r = build(flags)
    assert r is None, r.stderr[-4000:]
    print("multi_sim built %s" % ("with -fsanitize=address,undefined" if flags else "without sanitizers"))
    return {"dir": d, "flags": flags, "obj": obj, "exe": exe}


@pytest.fixture(scope="module")
def mutants(toolchain):
    """Every mutant built once, side by side: {name: (matches, build result, program)}."""
    text = open(MULTI).read()

    def make(name):
        old, new, _, _ = MUTANTS[name]
        d = toolchain["dir"] / name
        # multi.hip includes "../../include/sift_hip.h": give the copy the same surroundings
        (d / "include").mkdir(parents=True)
        (d / "include" / "sift_hip.h").write_text(open(os.path.join(ROOT, "include", "sift_hip.h")).read())
        (d / "sift-gpu_amd" / "csrc").mkdir(parents=True)
        src = d / "sift-gpu_amd" / "csrc" / "multi.hip"
        src.write_text(text.replace(old, new))
        mobj, exe = str(d / "multi.o"), str(d / "multi_sim")
        r = _run(BASE + toolchain["flags"] + ["-c", "-x", "c++", str(src), "-o", mobj])
        if r.returncode == 0:
            r = _run(BASE + toolchain["flags"] + [toolchain["obj"], mobj, "-o", exe])
        return text.count(old), r, exe

    with ThreadPoolExecutor(max_workers=min(len(MUTANTS), os.cpu_count() or 1)) as pool:
        return dict(zip(MUTANTS, pool.map(make, MUTANTS)))


def test_multi_hip_on_the_simulated_node(toolchain):
    """Every schedule x n in {1, 2, 3, 4, 8} x S in {1, 2, 3} x gather_desc, self
    p2p on and off at n = 1, 2, collecting every step and only after the flush;
    the capacity error at n = 2; both fault-injection sweeps."""
    r = _run([toolchain["exe"]])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    m = re.search(r"^multi sim ok: (\d+) configs, (\d+) schedules", r.stdout, re.M)
    assert m, r.stdout[-3000:]
    # 5 device counts x 3 x 2, self p2p doubling n = 1 and n = 2; 4 fixed schedules + 32 seeds
    assert (int(m.group(1)), int(m.group(2))) == (42, 36)
    assert "FAIL" not in r.stdout
    # the error paths at n = 2 ran: both sweeps injected a failure at every fallible call
    f = re.search(r"faults injected at (\d+) create and (\d+) steps \+ flush calls", r.stdout)
    assert f and int(f.group(1)) > 0 and int(f.group(2)) > 0, r.stdout[-3000:]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught(mutants, name):
    _, _, message, same_at_n1 = MUTANTS[name]
    matches, built, exe = mutants[name]
    assert matches == 1, "the text of mutant %s occurs %d times in multi.hip" % (name, matches)
    assert built.returncode == 0, built.stderr[-4000:]
    r = _run([exe])
    assert r.returncode != 0, "mutant %s passed:\n%s" % (name, r.stdout[-2000:])
    assert "multi sim ok" not in r.stdout
    assert re.search(r"^FAIL \[.*n=\d+ S=\d+ .*schedule=.* seed=\d+\]: " + message, r.stdout, re.M), \
        r.stdout[-3000:] + r.stderr[-3000:]
    if same_at_n1:
        # caught only with a second device: at n = 1 the mutant is the original program
        assert re.search(r"^FAIL \[\w+: n=[2-8] ", r.stdout, re.M), r.stdout[-3000:]
        r = _run([exe, "--n", "1"])
        assert r.returncode == 0 and "multi sim ok: 12 configs, 36 schedules" in r.stdout, \
            r.stdout[-3000:] + r.stderr[-3000:]
