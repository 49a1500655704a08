"""Timing of the pager stage (mfm_pocsag_process_device / mfm_flex_process_device / mfm_ais_process_device) on
resident PCM: idle channels (sync search only), busy channels (back-to-back POCSAG batches / FLEX frames / AIS packets)
and a mix.  One JSON line per scenario.

    python tools/bench_pager.py [--proto pocsag|flex|ais] [--channels 64] [--samples 699050] [--iters 20]

(FLEX: 699 050 samples at 25 kS/s are 447 392 at 16 kHz.  AIS: one 2^26-sample block at 2.4 MS/s is 1 398 101 samples
at 48 kHz; --samples defaults to that for --proto ais.)

    python tools/bench_pager.py --proto pocsag|ais --from-resampler pcm|bits|ab [--reps 6]

times resampler + stage as ONE unit on resident input PCM (--samples per channel at the resampler's input, 4/5, with the
low-pass the decoder tests use): `pcm` is mfm_resampler_process_device -> mfm_*_process_device, `bits` is
mfm_resampler_process_bits_device -> mfm_*_process_bits_device, `ab` times both on the same resident input, --reps times
each in rotating order after a warm-up, and prints mean, sd and the verdict of tools/exp/ab.py's rule (a difference counts
only beyond two standard errors of the difference) per scenario.  Every line carries the HBM bytes of one block computed
from the shapes (not measured).

Used for DESIGN.md section 9 and profiles/r01_pager_*; not part of bench.py's contract line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--proto", default="pocsag", choices=["pocsag", "flex", "ais"])
    ap.add_argument("--from-resampler", default=None, choices=["pcm", "bits", "ab"],
                    help="time resampler (4/5) + stage as one unit; ab: both forms alternating, with a verdict")
    ap.add_argument("--reps", type=int, default=6, help="--from-resampler: timed repetitions of --iters blocks per form")
    args = ap.parse_args()
    if args.from_resampler and args.proto == "flex":
        ap.error("--from-resampler is for --proto pocsag|ais: the FLEX stage needs the amplitudes")
    if not args.samples:
        args.samples = 1398101 if args.proto == "ais" else 699050
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    sy = pkg.synth
    C, n = args.channels, args.samples
    rng = np.random.RandomState(3)
    if args.from_resampler:
        return chain_main(pkg, torch, args.proto, args.from_resampler, C, n, args.iters, args.reps, rng)
    if args.proto == "flex":
        return flex_main(pkg, torch, C, n, args.iters, rng)
    if args.proto == "ais":
        return ais_main(pkg, torch, C, n, args.iters, rng)
    msgs = [(0x12345, 3, 2, sy.pocsag_alpha_words("THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789 " * 3 + "\x04"))] * 12
    bits = sy.pocsag_bits(sy.pocsag_batches(msgs))
    burst = {b: sy.pocsag_pcm(bits, b, noise=900, lead=3000, trail=3000, seed=b) for b in (512, 1200, 2400)}

    def busy(baud, seed):
        x = np.concatenate([burst[baud]] * (n // burst[baud].size + 1))[:n].copy()
        return x

    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([busy((512, 1200, 2400)[c % 3], c) for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        pg = pkg.Pocsag(C, n, device=0)
        for _ in range(3):
            pg.process_device(x.data_ptr(), n, n, stream=stream)
        nev = len(pg.fetch_events())
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.iters):
            pg.process_device(x.data_ptr(), n, n, stream=stream)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.iters
        print(json.dumps({"scenario": name, "channels": C, "pcm_samples_per_channel": n, "ms_per_block": round(ms, 4),
                          "pcm_msamples_per_s": round(C * n / ms / 1e3, 1), "events_last_block": nev,
                          "pcm_read_gbps": round(C * n * 2 / ms / 1e6, 1)}), flush=True)
        pg.close()


def flex_main(pkg, torch, C, n, iters, rng):
    sy = pkg.synth
    recs = [dict(kind="alnum", capcode=1000 + i, text="THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG %d" % i) for i in range(4)]
    frames = []
    for k in range(4):
        ph = {p: sy.flex_phase_words(recs) for p in sy.FLEX_CODINGS[k]["phases"]}
        frames.append(sy.flex_pcm([sy.flex_frame_levels(k, 1, k, ph)], noise=300, seed=k))
    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([np.concatenate([frames[c % 4]] * (n // 30000 + 2))[(c * 977) % 30000:][:n] for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        fx = pkg.Flex(C, n, device=0)
        for _ in range(3):
            fx.process_device(x.data_ptr(), n, n, stream=stream)
        ev, fw = fx.fetch_events()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fx.process_device(x.data_ptr(), n, n, stream=stream)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / iters
        print(json.dumps({"proto": "flex", "scenario": name, "channels": C, "pcm_samples_per_channel": n,
                          "ms_per_block": round(ms, 4), "pcm_msamples_per_s": round(C * n / ms / 1e3, 1),
                          "events_last_block": int(len(ev)), "frames_last_block": int(len(fw)),
                          "pcm_read_gbps": round(C * n * 2 / ms / 1e6, 1)}), flush=True)
        fx.close()


HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E, as bench.py


def ais_main(pkg, torch, C, n, iters, rng):
    """idle: noise only; busy: packets of types 1, 4, 5 back to back (one flag apart); mixed: every fourth channel
    busy.  Bytes read = the PCM once (2 bytes per sample), what the slicer must read; the bit planes the later kernels
    read and write are 1/8 and 2/8 of a byte per sample on top."""
    sy = pkg.synth
    pl = [sy.ais_type1(123456789, lon=-7234567, lat=2345678), sy.ais_type4(111222333),
          sy.ais_type5(987654321, callsign="TEST", ship_name="BENCH", destination="HBM")]
    train = sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(pl[k % 3]) for k in range(30)], gap_bits=0), noise=400, seed=1)
    idle = rng.normal(0, 1500, (C, n)).round().astype(np.int16)
    full = np.stack([np.concatenate([train] * (n // train.size + 2))[(c * 977) % train.size:][:n] for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(host).to(dev)
        st = pkg.Ais(C, n, device=0)
        for _ in range(3):
            st.process_device(x.data_ptr(), n, n, stream=stream)
        ev = st.fetch_events()
        torch.cuda.synchronize()
        reps = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                st.process_device(x.data_ptr(), n, n, stream=stream)
            t1.record()
            torch.cuda.synchronize()
            reps.append(t0.elapsed_time(t1) / iters)
        ms = float(np.median(reps))
        read = C * n * 2
        print(json.dumps({"proto": "ais", "scenario": name, "channels": C, "pcm_samples_per_channel": n,
                          "ms_per_block": round(ms, 4), "ms_reps": [round(r, 4) for r in reps],
                          "pcm_msamples_per_s": round(C * n / ms / 1e3, 1), "events_last_block": int(len(ev)),
                          "valid_packets_last_block": int(ev["fcs_valid"].sum()), "pcm_bytes_read": read,
                          "pcm_read_gbps": round(read / ms / 1e6, 1),
                          "frac_hbm_peak": round(read / ms / 1e6 / HBM_PEAK_GBPS, 3),
                          "realtime_factor": round(n / 48000.0 / (ms * 1e-3), 1)}), flush=True)
        st.close()


def chain_bytes(form, C, n_in, n_out):
    """HBM bytes of one block of resampler + stage, from the shapes: PCM in; then either PCM out and read back by the slicer
    and its bit plane written, or the bits written, read and written again by the splice (1/8 byte per output each)"""
    pcm_in, pcm_out, plane = C * n_in * 2, C * n_out * 2, C * ((n_out + 31) // 32) * 4
    return pcm_in + (2 * pcm_out + plane if form == "pcm" else 3 * plane)


def chain_main(pkg, torch, proto, form, C, n, iters, reps, rng):
    """resampler 4/5 + stage on resident input.  The scenarios are those of the stage benchmarks above (idle: noise, busy:
    back-to-back traffic, mixed: every fourth channel busy), made at the stage's rate and stretched by 5/4 (each sample
    repeated, every fourth kept) so that the resampler's output carries them; the low-pass is the one the decoder tests use
    (81 taps for POCSAG, tests/test_pocsag.py; 41 taps for AIS, the device-path test of tests/test_ais.py)."""
    import math
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    sy = pkg.synth
    n_stage = n * 4 // 5 + 8
    if proto == "pocsag":
        msgs = [(0x12345, 3, 2, sy.pocsag_alpha_words("THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG 0123456789 " * 3 + "\x04"))] * 12
        bits = sy.pocsag_bits(sy.pocsag_batches(msgs))
        trains = [sy.pocsag_pcm(bits, b, noise=900, lead=3000, trail=3000, seed=b) for b in (512, 1200, 2400)]
        taps = sy.design_lpf(81, 0.45 / 5, 1.0) * 4
        pol = pkg.binding.MFM_BITS_NEG
    else:
        pl = [sy.ais_type1(123456789, lon=-7234567, lat=2345678), sy.ais_type4(111222333),
              sy.ais_type5(987654321, callsign="TEST", ship_name="BENCH", destination="HBM")]
        trains = [sy.ais_pcm(sy.ais_bits([sy.ais_frame_bits(pl[k % 3]) for k in range(30)], gap_bits=0), noise=400, seed=1)]
        taps = sy.design_lpf(41, 0.45 / 5, 1.0) * 4
        pol = pkg.binding.MFM_BITS_POS
    rtaps = oracle_lib.quantize_taps(taps)

    def stretch(x):
        return np.repeat(x, 5)[::4][:n]

    busy_rows = [stretch(np.concatenate([t] * (n_stage // t.size + 2))[:n_stage]) for t in trains]
    idle_pool = stretch(rng.normal(0, 1500, n_stage + 4096).round().astype(np.int16)[:n_stage])
    idle = np.stack([np.roll(idle_pool, 977 * c) for c in range(C)])
    full = np.stack([np.roll(busy_rows[c % len(busy_rows)], 0 if proto == "pocsag" else 977 * c) for c in range(C)])
    mix = idle.copy()
    mix[::4] = full[::4]
    stream = torch.cuda.current_stream().cuda_stream
    forms = ["pcm", "bits"] if form == "ab" else [form]
    Stage = pkg.Pocsag if proto == "pocsag" else pkg.Ais
    for name, host in (("idle", idle), ("busy", full), ("mixed", mix)):
        x = torch.from_numpy(np.ascontiguousarray(host)).to(torch.device("cuda:0"))
        objs, n_out, nev = {}, {}, {}
        for f in forms:
            rs = pkg.Resampler(C, rtaps, 4, 5, n, device=0)
            objs[f] = (rs, Stage(C, rs.max_out(), device=0))

        def block(f):
            rs, st = objs[f]
            if f == "pcm":
                yptr, ystride, ny = rs.process_device(x.data_ptr(), n, n, stream=stream)
                st.process_device(yptr, ystride, ny, stream=stream)
                return ny
            v = rs.process_bits_device(x.data_ptr(), n, n, pol, stream=stream)
            st.process_bits_device(v, stream=stream)
            return v.nr_bits

        for f in forms:  # warm-up
            for _ in range(3):
                n_out[f] = block(f)
            nev[f] = int(len(objs[f][1].fetch_events()))
        torch.cuda.synchronize()
        ms = {f: [] for f in forms}
        for r in range(reps):
            for f in (forms if r % 2 == 0 else forms[::-1]):  # rotating order
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(iters):
                    block(f)
                t1.record()
                torch.cuda.synchronize()
                ms[f].append(t0.elapsed_time(t1) / iters)
        stat = {}
        for f in forms:
            m = sum(ms[f]) / len(ms[f])
            sd = math.sqrt(sum((v - m) ** 2 for v in ms[f]) / (len(ms[f]) - 1)) if len(ms[f]) > 1 else float("nan")
            stat[f] = (m, sd)
            nbytes = chain_bytes(f, C, n, n_out[f])
            print(json.dumps({"proto": proto, "from_resampler": f, "scenario": name, "channels": C, "in_samples_per_channel": n,
                              "out_samples_per_channel": n_out[f], "ms_per_block": round(m, 4), "ms_sd": round(sd, 4),
                              "ms_reps": [round(v, 4) for v in ms[f]], "events_last_block": nev[f],
                              "hbm_bytes_from_shapes": nbytes, "gbps_from_shapes": round(nbytes / m / 1e6, 1)}), flush=True)
        if form == "ab":
            (bm, bs), (m, sd) = stat["pcm"], stat["bits"]
            d, se = m - bm, math.sqrt(sd * sd / reps + bs * bs / reps)
            verdict = "neutral" if abs(d) <= 2.0 * se else ("kept" if d < 0 else "worse")
            print(json.dumps({"proto": proto, "scenario": name, "channels": C, "ab": "bits vs pcm", "verdict": verdict,
                              "delta_percent": round(100.0 * d / bm, 2), "delta_in_se": round(abs(d) / se, 1) if se > 0 else None,
                              "same_event_count": nev["pcm"] == nev["bits"]}), flush=True)
        for rs, st in objs.values():
            st.close()
            rs.close()


if __name__ == "__main__":
    main()
