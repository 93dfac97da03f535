#!/usr/bin/env python3
"""Generate tests/golden/landscapes.npz from the COMPILED REFERENCE (oracle/_ref/libslamref.so, `make -C oracle ref`): the
decisions of BruteForceScanMatcher, HillClimbingScanMatcher and MonteCarloScanMatcher
(src/core/scan_matchers/pose_enumeration_scan_matcher.h:31-77) on the designed score tables of tests/landscape_cases.py.

    python tests/golden/make_golden_landscapes.py

Per case the table is written cell by cell through GridMap::update into an UnboundedPlainGridMap of MockGridCell (its
operator+= stores the observation's occupancy as it is), exported again and compared with the designed table bit for bit;
the scan is one beam of the case's range at heading 0 behind the raw trig provider, scored by the obstacle OOPE under the
discrepancy OIE with even weights; the case's matches run in order on ONE matcher object.  Asserted per match: one point
left by the matcher's scan filter, for brute force the walk's nx, ny, nt read back from the trace, the author's expected
decision (landscape_cases.accept_loop) for BF and HC, the margin of the drawn MC poses.

One row per match, named KIND:case#k: n_calls, prob, delta, the accepted call indices, the SHA-256 of the scores and of the
poses (not the traces themselves).  A case with NaN in its table is tried in a forked child first: where the reference
refuses it (an assertion of its own ends the child), the case is listed in `refused` and has no rows -- the CPU oracle
alone answers for it.  No case without NaN may be refused.  The file is a function of this script and
tests/landscape_cases.py alone: the archive's time stamps are fixed, two runs give the same bytes."""
import hashlib
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

GOLDEN_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLDEN_DIR))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pyoracle import *  # noqa: E402,F401,F403
import landscape_cases as lc  # noqa: E402

KINDS = dict(BF=SM_BF, HC=SM_HC, MC=SM_MC)
MAX_BYTES = 300 * 1024


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def run_case(R, c):
    """the case's matches on the reference: a list of traces"""
    h, w = c.payload.shape
    m = R.map_create(REF_CELL_MOCK, MAP_UNBOUNDED_PLAIN, w, h, lc.S, lc.PROTO)
    for j, i in np.argwhere(lc.bits(c.payload) != lc.bits(np.array(lc.PROTO))):
        m.update(int(i) - c.origin[0], int(j) - c.origin[1], float(c.payload[j, i]))
    md = m.to_data()
    assert (md.width, md.height, md.origin, md.scale) == (w, h, tuple(c.origin), lc.S), c.name
    assert np.array_equal(lc.bits(md.payload[:, :, 0]), lc.bits(c.payload)), c.name + ": the exported table differs"
    assert lc.bits(md.unknown[:1])[0] == lc.bits(np.array(lc.PROTO))
    scan = R.scan_create([c.rng], [0.0], [1])
    spe = R.spe_create(OOPE_OBSTACLE, OIE_DISCREPANCY, 0)
    fs = R.filter_scan(spe, scan, c.inits[0], m)  # (EvenSPW takes its weight from the scan the estimator filtered)
    assert fs.size() == 1 and np.array_equal(R.scan_weights(spe, fs), [1.0]) and np.array_equal(fs.get()[3], [1.0])
    matcher = R.matcher_create(KINDS[c.kind], spe, c.params)
    out = []
    for k, init in enumerate(c.inits):
        t = R.process_scan(matcher, scan, init, m, cap=1 << 16)
        assert t["filtered_n"] == 1 and t["n_calls"] <= 1 << 16, c.name
        if c.kind == "BF":
            walk = t["poses"][1:]
            assert tuple(len(np.unique(walk[:, d])) for d in range(3)) == c.shape, c.name
            assert t["n_calls"] == 1 + c.shape[0] * c.shape[1] * c.shape[2]
        if c.expect is not None:
            want = c.expect[k]
            assert t["n_calls"] == want["n_calls"], (c.name, t["n_calls"], want["n_calls"])
            assert np.nonzero(t["accepted"])[0].tolist() == want["accepted"], c.name
            assert np.array_equal(t["poses"][want["win"]] - init, t["delta"]), c.name
            assert lc.bits(t["scores"][want["win"]]) == lc.bits(t["prob"]), c.name
        else:
            assert lc.margin_holds(c.payload, c.origin, t["poses"], c.rng, lc.DRAWN_MARGIN), c.name
        out.append(t)
    return out


def survives(R, c):
    """whether the reference runs the case without one of ITS assertions (which ends the forked child with SIGABRT); a
    check of this script that fails in the child is an error, not a refusal"""
    sys.stdout.flush()
    pid = os.fork()
    if pid == 0:
        os.dup2(os.open(os.devnull, os.O_WRONLY), 2)
        try:
            run_case(R, c)
        except BaseException:
            os._exit(3)
        os._exit(0)
    status = os.waitpid(pid, 0)[1]
    assert status == 0 or os.WIFSIGNALED(status), c.name + ": a check of the generator failed"
    return status == 0


def write_npz(path, out):
    """np.savez_compressed with the members in sorted order and a fixed time stamp"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    if not ref_available():
        sys.exit("oracle/_ref/libslamref.so missing: run `make -C oracle ref` where the reference tree exists")
    so = os.path.join(ROOT, "oracle", "_ref", "libslamref.so")
    assert "__assert_fail" in subprocess.check_output(["nm", "-D", "--undefined-only", so]).decode(), \
        "the reference was compiled without its assertions"
    R = Ref()
    names, n_calls, prob, delta, s_sha, p_sha, acc, off, refused = [], [], [], [], [], [], [], [0], []
    for c in lc.all_cases():
        if np.any(np.isnan(c.payload)) and not survives(R, c):
            refused.append(c.kind + ":" + c.name)
            print("refused by the reference:", refused[-1])
            continue
        for k, t in enumerate(run_case(R, c)):
            names.append("%s:%s#%d" % (c.kind, c.name, k))
            n_calls.append(t["n_calls"])
            prob.append(t["prob"])
            delta.append(t["delta"])
            s_sha.append(sha(t["scores"]))
            p_sha.append(sha(t["poses"]))
            acc.append(np.nonzero(t["accepted"])[0])
            off.append(off[-1] + len(acc[-1]))
    out = dict(names=np.array(names), n_calls=np.array(n_calls, np.int32), prob=np.array(prob), delta=np.array(delta),
               scores_sha256=np.array(s_sha), poses_sha256=np.array(p_sha), accepted_idx=np.concatenate(acc).astype(np.int32),
               accepted_off=np.array(off, np.int64), refused=np.array(refused, dtype="U80"))
    path = os.path.join(GOLDEN_DIR, "landscapes.npz")
    write_npz(path, out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, size
    print("wrote landscapes.npz %d KiB: %d matches of %d cases, %d refused, sha256 %s"
          % (size // 1024, len(names), len(lc.all_cases()), len(refused), hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]))


if __name__ == "__main__":
    main()
