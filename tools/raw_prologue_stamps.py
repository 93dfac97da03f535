"""In-kernel timeline of the lone co-resident hill-climbing chain behind slamhip_matcher_process_raw_scan
(csrc/hc_resident.hip), with the chain assembling the raw scan in its prologue (SLAMHIP_OPT_RAW_PROLOGUE 1) and behind
the assembly kernel (0): kernel begin -> first super-step's start, and the later super-steps' phases, of one scoring
workgroup.  Run on the GPU box."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from synth import cast_scan, make_scene  # noqa: E402

pkg = ge.load_package()
ctx = pkg.Context(0, testing=True)  # (the stamps are a hook of libslamhip_testing.so)
sc = make_scene(cell_model=0, size=2000, scale=0.05, n_beams=1080, seed=100)
ctx.upload_map(0, sc["map"])
rng, ang, occ = cast_scan(sc["gt"], sc["map"].scale, sc["true_pose"], 1080, seed=5, raw=True)
L = pkg.load(testing=True)
L.slamhip_matcher_debug_stamps.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
has_option = hasattr(pkg, "OPT_RAW_PROLOGUE")  # (a build from before the option: the assembly kernel, always)
for threads in (1024, 512, 256):
    for opt in ((1, 0) if has_option else (0,)):
        if has_option:
            ctx.set_option(pkg.OPT_RAW_PROLOGUE, opt)
        m = pkg.Matcher(ctx, "HC", pkg.spe_cfg(), [128, 0.1, 0.1])
        m.set_device_chain(2, threads)
        match = m.make_raw_process_scan(0, rng, ang, is_occ=occ)
        rows = []
        for rep in range(12):
            if rep == 4:
                L.slamhip_matcher_debug_stamps(m.h, None)
            kept, _ = match(sc["init_pose"])
            if rep >= 4:
                buf = (C.c_longlong * 512)()
                L.slamhip_matcher_debug_stamps(m.h, buf)
                st = np.array(list(buf)).reshape(64, 8)[:min(m.stats()["launches"], 64)]
                rows.append(st)
        pro = np.array([(st[0, 0] - st[0, 6]) / 100.0 for st in rows]) if has_option else np.array([np.nan])
        first = np.array([(st[0, 5] - st[0, 0]) / 100.0 for st in rows])
        step = np.array([(np.diff(st[:, 0]) / 100.0)[1:].mean() for st in rows])
        step1 = np.array([(st[2, 0] - st[1, 0]) / 100.0 for st in rows])
        print("threads %4d, raw prologue %d, %d beams kept: kernel begin -> first super-step %.2f us (min %.2f, max %.2f); first "
              "super-step, start -> score stored %.2f; super-step 1 %.2f; later super-steps %.2f us each; resident %r" %
              (threads, opt, kept, np.median(pro), pro.min(), pro.max(), np.median(first), np.median(step1), np.median(step),
               m.resident_stats()))
        m.close()
