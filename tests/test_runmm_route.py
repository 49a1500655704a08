"""The burst Mueller-Muller stage behind the run router: a route of its own beside a POCSAG route, one gate in front of both.
Each route's output equals the chain run alone on the gate's own view, filtered to the route's channels, and the oracle's
(tests/test_runmm.py's Checker, tests/test_runpocsag.py's) on the filtered run list.  Every comparison is an equality."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_runmm as trm
import test_runpocsag as trp
import test_runroute as trr
import test_runrs as tr

ROUTED = dict(W=64, P=1, hang=2, ratio=(4, 5, 41), seed=23)
PAR = dict(kw=trm.KW, km=trm.KM, spb=16.0, emin=float(np.float32(16.0) - trm.MARGIN), emax=float(np.float32(16.0) + trm.MARGIN))


class MmChain:
    """burst resampler -> burst Mueller-Muller stage on the device, behind whatever view it is given"""

    def __init__(self, pkg, nch, taps, ratio, W, cap, P):
        self.rr = pkg.RunResampler(nch, taps, ratio[0], ratio[1], W, max_in_samples=cap, preroll_windows=P)
        self.st = pkg.RunMm.behind(self.rr, PAR["spb"], PAR["kw"], PAR["km"], error_min=PAR["emin"], error_max=PAR["emax"])

    def call(self, view):
        self.rr.process_device(*view)
        self.st.process_device(*self.rr.device_view())
        return self.rr.fetch(), self.st.fetch()

    def close(self):
        self.st.close()
        self.rr.close()


@pytest.mark.gpu
def test_gpu_an_mm_route_beside_a_pocsag_route(pkg, ora):
    """one level and one gate (P = 1) over the four rows of the short POCSAG scene in ragged calls and the flush; route 0 a
    Mueller-Muller chain at 4/5 on channels 0 and 1, route 1 a POCSAG chain at 4/5 on channels 2 and 3"""
    b = pkg.binding
    s = ROUTED
    W, P, (I, D, _) = s["W"], s["P"], s["ratio"]
    rows = np.ascontiguousarray(trp.scene(pkg, ora, s["ratio"], 7)["stream"])
    n = rows.shape[1]
    taps = trp.rs_taps(pkg, ora, s["ratio"])
    table = np.array([0, 0, 1, 1], np.uint8)
    rng = np.random.RandomState(s["seed"])
    cuts = [0]
    while sum(cuts) < n:
        cuts.append(min(int(rng.randint(1, 7001)), n - sum(cuts)))
    nch, cap, thr = rows.shape[0], max(cuts), W * 1000 * 1000
    lv = pkg.Level(nch, cap, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, hang_windows=s["hang"])
    gate = pkg.Gate(nch, cap, W, preroll_windows=P)
    router = pkg.RunRouter.behind(table, 2, cap, W, preroll_windows=P)
    routed = [MmChain(pkg, nch, taps, (I, D), W, cap, P), trr.Chain(pkg, nch, taps, (I, D), W, cap, P, "pocsag")]
    plain = [MmChain(pkg, nch, taps, (I, D), W, cap, P), trr.Chain(pkg, nch, taps, (I, D), W, cap, P, "pocsag")]
    chk = [trm.Checker(pkg, ora, PAR), trp.Checker(pkg, ora, taps, I, D, W)]
    rs = tr.Checker(pkg, ora, taps, I, D, False, W)
    pos, decisions, events = 0, 0, 0
    for i, m in enumerate(cuts + [None]):
        if m is not None:
            gr, gp = gate.process_host(rows[:, pos:pos + m], lv.process_host(rows[:, pos:pos + m]))
            pos += m
        else:
            gate.flush_device()
            gr, gp = gate.fetch()
        router.process_device(*gate.device_view())
        # route 0: clock recovery
        what = f"call {i}, the mm route"
        mine = trr.filtered(gr, table, 0)
        (runs, payload), (mruns, dec) = routed[0].call(router.device_view(0))
        (all_runs, all_payload), (all_mruns, all_dec) = plain[0].call(gate.device_view())
        keep = table[all_runs["channel"]] == 0
        trr.same_but(runs, all_runs[keep], ("out_offset",), what)
        trr.same_but(mruns, all_mruns[keep], ("dec_offset",), what)
        assert np.array_equal(mruns["dec_offset"], np.cumsum(mruns["nr_dec"], dtype=np.uint64) - mruns["nr_dec"]), what
        for a, o in zip(mruns, all_mruns[keep]):
            assert np.array_equal(dec[int(a["dec_offset"]):int(a["dec_offset"]) + int(a["nr_dec"])],
                                  all_dec[int(o["dec_offset"]):int(o["dec_offset"]) + int(o["nr_dec"])]), what
        want_rs = rs.call(mine, gp)
        tr.same((runs, payload), want_rs, what)
        trm.same((mruns, dec), chk[0].call(*want_rs), what)
        decisions += dec.size
        # route 1: POCSAG, as it was without a neighbour
        what = f"call {i}, the pocsag route"
        (runs, payload), ev = routed[1].call(router.device_view(1))
        (all_runs, all_payload), all_ev = plain[1].call(gate.device_view())
        trr.same_but(ev, all_ev[table[all_ev["channel"]] == 1], ("run",), what)
        (rs_want, rs_payload), ev_want = chk[1].call(trr.filtered(gr, table, 1), gp)
        trp.same(ev, ev_want, what)
        tr.same((runs, payload), (rs_want, rs_payload), what)
        events += len(ev)
    by = chk[0].stretches()
    assert pos == rows.shape[1] and {k[0] for k in by} <= {0, 1} and len(by) >= 2 and decisions == sum(d.size for d in by.values()) >= 200 and events >= 2
    assert {k[0] for k in chk[1].stretches()} <= {2, 3}
    for o in routed + plain + [router, gate, lv]:
        o.close()


@pytest.mark.gpu
def test_gpu_level_scan_tool_with_an_mm_route_writes_what_gate_mm_writes(pkg, ora, tmp_path):
    """tools/level_scan.py --gate-route FILE as a fresh child process on the chain scene of tests/test_runpocsag.py, a route of
    stage mm on channel 0 beside a POCSAG route on channel 1, then the mm route on both: DIR/<name>/chNNNN.mm.s16 and mm.jsonl hold
    the oracle's decisions of the route's channels, with the configuration's channel numbers, as --gate-mm writes them"""
    base = trm.tool_setup(pkg, ora, tmp_path)
    by, W = trm.tool_want(pkg, ora), trp.CHAIN["W"]
    taps = str(tmp_path / "filter.json")
    for name, doc, channels in (
            ("beside", {"routes": [{"name": "sym", "stage": "mm", "resample": "4/5", "taps": taps, "channels": [1], "mm": {"spb": 16}},
                                   {"name": "pg", "stage": "pocsag", "resample": "4/5", "taps": taps, "channels": [0]}]}, (1,)),
            ("local", {"local": True, "routes": [{"name": "sym", "stage": "mm", "resample": "4/5", "taps": taps, "channels": [0, 1],
                                                  "mm": {"spb": 16.0, "kw": trm.KW, "km": trm.KM, "margin": 0.05}}]}, (0, 1))):
        (tmp_path / (name + ".json")).write_text(json.dumps(doc))
        r = subprocess.run(base + ["--gate-out", str(tmp_path / name), "--gate-route", str(tmp_path / (name + ".json"))],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        trm.tool_check(tmp_path / name / "sym", by, W, channels)
    assert (tmp_path / "beside" / "pg" / "pocsag.jsonl").read_text().count("\n") >= 3


ROUTE_REFUSALS = [
    ({"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0]}, "\"mm\" must be an object of numbers with spb"),
    ({"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"kw": 1.0}}, "\"mm\" must be an object of numbers with spb"),
    ({"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"spb": "16"}}, "\"mm\" must be an object of numbers with spb"),
    ({"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"spb": 16, "gain": 1}}, "\"mm\" must be an object of numbers with spb"),
    ({"name": "a", "stage": "mm", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"spb": 16}, "bits": True},
     "bits needs stage ais or pocsag: the burst Mueller-Muller stage reads PCM values"),
    ({"name": "a", "stage": "pocsag", "resample": "4/5", "taps": "f.json", "channels": [0], "mm": {"spb": 16}}, "\"mm\" belongs to stage mm, not to stage pocsag"),
]


@pytest.mark.parametrize("route,message", ROUTE_REFUSALS, ids=[str(i) for i in range(len(ROUTE_REFUSALS))])
def test_level_scan_tool_refuses_a_bad_mm_route_before_it_sets_anything_up(tmp_path, route, message):
    """what is wrong with a route of stage mm ends the run with a message, before a device is looked for; so do the flags that
    do not go with --gate-mm"""
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}, {"chanCenterFreq": 928900000}]}))
    (tmp_path / "routes.json").write_text(json.dumps({"routes": [route]}))
    tool = [sys.executable, os.path.join(trm.ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", str(tmp_path / "none.bin")]
    r = subprocess.run(tool + ["--gate-out", str(tmp_path / "out"), "--gate-route", str(tmp_path / "routes.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and message in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "out").exists()


def test_level_scan_tool_refuses_what_does_not_go_with_gate_mm(tmp_path):
    (tmp_path / "rx.json").write_text(json.dumps({"sampleRateHz": 1200000, "centerFreqHz": 929000000, "decimationFactor": 25, "lpfTaps": [1.0],
                                                  "channels": [{"chanCenterFreq": 929100000}]}))
    tool = [sys.executable, os.path.join(trm.ROOT, "tools", "level_scan.py"), "--config", str(tmp_path / "rx.json"), "--input", str(tmp_path / "none.bin"),
            "--gate-out", str(tmp_path / "out")]
    rs = ["--gate-resample", "4/5", "--resample-taps", "f.json"]
    for flags, message in ((["--gate-mm", "16"], "--gate-mm needs --gate-resample"),
                           (rs + ["--gate-mm", "16", "--gate-flex"], "--gate-mm, --gate-flex, --gate-pocsag and --gate-ais exclude each other"),
                           (rs + ["--gate-mm", "16", "--gate-bits"], "--gate-mm and --gate-bits exclude each other"),
                           (rs + ["--gate-mm", "16", "--gate-ends"], "--gate-mm and --gate-ends exclude each other"),
                           (rs + ["--gate-mm", "16,0.1"], "--gate-mm takes SPB or SPB,KW,KM,MARGIN"),
                           (rs + ["--gate-mm", "fast"], "--gate-mm takes SPB or SPB,KW,KM,MARGIN"),
                           (["--gate-mm", "16", "--gate-route", "r.json"], "--gate-route excludes --gate-mm")):
        r = subprocess.run(tool + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and message in r.stderr, (flags, r.stderr[-2000:])
    assert not (tmp_path / "out").exists()
