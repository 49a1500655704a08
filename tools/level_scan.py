#!/usr/bin/env python3
"""Which channels of a capture carry a signal: channel engine, then the level / squelch stage, both on the device.

    python tools/level_scan.py --config receiver.json --input capture.bin [--format cs16|cs8|cu8] [--form pcm|iq]
           [--window 1000] [--metric energy|diff] [--sense above|below] [--open-thr N --close-thr N] [--hang 0]
           [--floor-windows M --open-ratio R --close-ratio R [--warmup N]]
           [--block 1048576] [--summary] [--gate-out DIR [--gate-preroll P] [--gate-resample I/D --resample-taps FILE [--gate-dc-pole POLE]
           [--gate-ais | --gate-pocsag | --gate-flex | --gate-mm SPB[,KW,KM,MARGIN] [--gate-sync WORDS [--gate-batch [KEEP[,BAUD]]]]]] | --gate-route routes.json]]

receiver.json has the reference's shape (multifm/receiver.c:138-230): sampleRateHz, centerFreqHz, decimationFactor,
lpfTaps, channels[].chanCenterFreq (and the optional dBGain).  One JSON line per channel and completed window:

    {"freq": 929612500, "channel": 0, "window": 3, "energy": ..., "diff_energy": ..., "peak": ..., "open": 1}

--form pcm runs the stage on the discriminator's PCM (a captured carrier LOWERS its energy: default sense below),
--form iq on the filtered IQ (a carrier RAISES it: default sense above).  --summary adds one line per channel with the
share of windows it was open.  The thresholds default to 0: read the levels off a first run, then set them - or let every
channel follow its own noise floor:

--floor-windows M --open-ratio R --close-ratio R [--warmup N] switch the adaptive squelch on (mfm_level_set_adaptive): the floor
of a window is the smallest (sense above; the largest with sense below) metric of the channel's last M windows, that window
included; a channel opens at R times its floor and a window is bad beyond the close ratio (R as a float, taken in 1/256:
round(256 R)), and the first N windows open nothing.  --open-thr / --close-thr stay in force as absolute limits (with sense
below and none given they are set to 2^64 - 1, no limit).  Every record line then carries "floor" behind "open", and a --summary
line "median_floor", the lower median of the channel's floors.

--gate-out DIR queues the gate stage behind the level stage on the engine's stream, on the rows the scan runs on (PCM, or
IQ with --form iq): only the windows the squelch left open leave the device.  Per channel that ever opened DIR/chNNNN.s16
gets the gated samples, and DIR/index.jsonl one line per run:

    {"channel": 3, "first_sample": 4000, "nr_samples": 2000, "file_offset": 0}

(first_sample and nr_samples in samples of the channel, file_offset in bytes of its file).  What goes to stdout does not change.
--gate-preroll P (default 0) also lets the P windows in front of every opening through (window k goes out when any of the
records k .. k + P is open): the gate's output then comes P windows late, and at the end of the input the gate is flushed and
the runs the flush brings are written like any others.

--gate-resample I/D --resample-taps FILE (with --gate-out and --form pcm) queues the burst resampler behind the gate on the same
stream: every stretch of consecutive gated windows of a channel goes through a fresh rational resampler I/D whose taps are FILE's
"lpfCoeffs" (quantised to Q14 as the decoder does).  Beside the gated files DIR/chNNNN.rs.s16 gets the channel's resampled
samples and DIR/resampled.jsonl one line per run:

    {"channel": 3, "first_sample": 4000, "first_out": 0, "nr_out": 1597, "begins": 1, "file_offset": 0}

(first_sample in samples of the channel at the input rate, first_out the index of the run's first output within its stretch,
begins 1 on a stretch's first run, file_offset in bytes of the .rs.s16 file).

--gate-dc-pole POLE (with --gate-resample; the decoder's -b -p POLE) switches on the burst resampler's DC blocker: every stretch's
resampled samples go through a fresh DC blocker with that pole, on the device, before they are written or read by the stage
behind - --gate-ais, --gate-pocsag and --gate-flex see the blocked PCM with no change of their own.  A receiver tuned off a
carrier by more than the deviation needs it: the sign of the samples is all the AIS and POCSAG slicers look at.  Not together
with --gate-bits: the blocker filters the PCM the sign bits would be taken from.

--gate-ais (with --gate-resample) queues the burst AIS stage behind the burst resampler on the same stream, the flush call
included: every stretch goes through a fresh AIS demodulator, and DIR/ais.jsonl gets one line per candidate packet:

    {"channel": 3, "first_sample": 4000, "sample": 2549, "start_sample": 1575, "nr_bytes": 23, "fcs_valid": 1, "bytes": "0465..."}

(first_sample: where the packet's stretch begins, in samples of the channel at the input rate; sample and start_sample: the
resampled samples, counted from the stretch's first, where the packet ended and where its preamble matched; bytes: nr_bytes
bytes as hex, the FCS included).

--gate-pocsag (with --gate-resample whose output rate is 38 400 Hz; not together with --gate-ais) queues the burst POCSAG stage
behind the burst resampler on the same stream, the flush call included: every stretch goes through a fresh POCSAG demodulator.
DIR/pocsag.jsonl gets one line per event:

    {"channel": 3, "first_sample": 4000, "type": 2, "baud": 1200, "sample": 26999, "aux": 0, "nr_ok": 16, "fail_mask": 0,
     "corrected": ["7a89c197", ...]}

(first_sample: where the event's stretch begins, in samples of the channel at the input rate; type: MFM_POCSAG_EV_*; sample: the
resampled sample, counted from the stretch's first, that completed the event; corrected: the 16 words of a BATCH as hex, empty
otherwise).  DIR/pages.jsonl gets the pages a fresh host pager per stretch (host/mfm_pager_pocsag.c, through libmfm_host.so)
assembles from the events, in the shape decoder_amd prints them, with the channel and the stretch in the place of the time:

    {"proto": "pocsag", "type": "alphanumeric", "channel": 3, "first_sample": 4000, "baud": 1200, "capCode": 596523, "function": 2,
     "message": "HELLO"}

--gate-flex (with --gate-resample whose output rate is 16 000 Hz; not together with --gate-ais or --gate-pocsag) queues the burst
FLEX stage behind the burst resampler on the same stream, the flush call included: every stretch goes through a fresh FLEX
decoder.  DIR/flex.jsonl gets one line per event:

    {"channel": 3, "first_sample": 4000, "type": 1, "sample": 31204, "sync_sample": 2642, "coding": 2, "baud": 3200, "eye": 10,
     "a": 1335318841, "b": 21845, "inv_a": 2959648454, "fiw_raw": 2820680286, "fiw": 673196638, "fiw_rc": 0, "sample_range": 18001,
     "sample_delta": 1, "cycle": 5, "frame": 42, "nr_phases": 2}

(first_sample as above; type: MFM_FLEX_EV_*; sample and sync_sample: resampled samples counted from the stretch's first; the rest
are the fields of mfm_flex_event).  DIR/pages.jsonl gets the messages a fresh host FLEX pager per stretch (host/mfm_pager_flex.c,
through libmfm_host.so) assembles from the frames' words, in the shape decoder_amd prints them, with the channel and the stretch in
the place of the time:

    {"proto": "flex", "type": "alphanumeric", "channel": 3, "first_sample": 4000, "baud": 3200, "frameNo": 42, "cycleNo": 5,
     "phaseNo": "A", "capCode": 123456, "fragment": false, "maildrop": false, "fragSeq": 3, "message": "HELLO"}

--gate-mm SPB[,KW,KM,MARGIN] (with --gate-resample; beside no other stage flag, --gate-bits or --gate-ends) queues the burst
Mueller-Muller stage behind the burst resampler on the same stream, the flush call included: every stretch goes through a fresh
clock recovery loop mm_init(KW, KM, SPB, SPB - MARGIN, SPB + MARGIN) (pager/mueller_muller.c; SPB is samples per bit at the
resampler's output rate, the other three default to the reference test's 0.0001, 0.000004 and 0.05; all are taken as float32).
DIR/chNNNN.mm.s16 gets the channel's decisions - the samples the loop picked, one per recovered symbol - appended, and DIR/mm.jsonl
one line per run:

    {"channel": 3, "first_sample": 4000, "first_dec": 0, "nr_dec": 76, "begins": 1, "file_offset": 0}

(first_sample: the run's first sample, in samples of the channel at the input rate; first_dec the index of the run's first decision within its stretch,
begins 1 on a stretch's first run, file_offset in bytes of the .mm.s16 file).  It is the product for a 2-FSK channel none of the
three decoders understands: d > 0 ? 0 : 1 is the reference consumer's bit.

    python tools/level_scan.py --bench-runmm --window 4096 [--reps 8] [--inner 10]

prints one line ("runmm_stage"): burst resampler -> burst Mueller-Muller stage on a gate's device view against mfm_resampler ->
mfm_mm on the full rows, 4/5 with 41 taps, 131 072 input samples per channel at 64 and 1024 channels, the three masks all-closed,
scene (a squelch at the median window energy) and all-open, the two chains alternating in one process in rotating order; and
whether a sample of the burst decisions (the first runs of a call) equalled the host twin's.

--gate-sync WORD[,WORD...][/DIST][,either] (only with --gate-mm) queues the burst sync stage (mfm_runsync_*) behind the burst
Mueller-Muller stage on the same stream: per stretch a fresh 32-bit register takes d > 0 ? 0 : 1 of every decision
(pager/test/test_mueller_muller.c:130-136), and wherever it is within DIST bits (default 3, at most 15) of one of the one to eight
words - with ",either" of a word's complement too - DIR/sync.jsonl gets a line:

    {"channel": 3, "first_window": 4, "first_sample": 4000, "dec": 331, "word": "7cd215d8", "distance": 0, "inverted": 0, "seen": "7cd215d8"}

(first_window and first_sample: where the stretch began; dec: the decision that completed the word, counted within the stretch), and
once a stretch is over - the channel's next one begins, or the run ends - a summary line with its decisions and the count per word:

    {"channel": 3, "first_window": 4, "first_sample": 4000, "decisions": 1210, "events": {"7cd215d8": 2}}

A route of stage mm may carry "sync": {"words": [2094142936], "distance": 3, "either": false} with the same meaning (words required).
Without the flag nothing the tool writes changes.

    python tools/level_scan.py --bench-runsync --window 4096 [--reps 6] [--inner 10]

prints one line ("runsync_stage"): the chain of --bench-runmm with and without the sync stage behind it, and the resampler alone, on
the same three masks at 64 and 1024 channels, alternating in one process: means, standard deviations, the sync stage's cost as
the difference with its standard error and the verdict of tools/exp/ab.py's two-standard-error rule, and that cost over the
Mueller-Muller stage's own call (the chain minus the resampler); and whether every call's result equalled the host twin's.

--gate-batch [KEEP[,BAUD]] (only with --gate-sync) queues the burst batch stage (mfm_runbatch_*) behind the burst sync stage on the
same stream: behind a sync event it cuts batches of 16 codewords out of the sync stage's bit words, runs BCH(31,21) on them and
holds the 32 bits behind every batch against the word that was found, within KEEP bits (default 4, at most 15), as
pager/pager_pocsag.c:468-538 does at one sample per bit.  DIR/batch.jsonl gets a line per event:

    {"channel": 3, "first_window": 4, "first_sample": 4000, "type": 2, "dec": 843, "aux": "00000000", "word": "7cd215d8", "inverted": 0,
     "nr_ok": 16, "fail_mask": 0, "corrected": ["7a89c197", ...]}

(type: MFM_POCSAG_EV_*, 1 sync found, 2 batch, 3 sync lost, 4 sync kept; dec: the decision that completed the event, counted within
the stretch; corrected only on a batch), and the pages of a fresh host pager per stretch go to DIR/pages.jsonl in the shape
--gate-pocsag writes, with BAUD (default 1200: the stage counts decisions and does not know the rate) in the place of the baud rate.
A route of stage mm that carries "sync" may carry "batch": {"keep": 4, "baud": 1200} with the same meaning (both optional).

    python tools/level_scan.py --bench-runbatch --window 4096 [--reps 6] [--inner 10]

prints one line ("runbatch_stage"): the chain of --bench-runsync with and without the batch stage behind it on the same three masks
at 64 and 1024 channels, alternating in one process in rotating order: means, standard deviations, the batch stage's cost as the
difference with its standard error and the verdict of tools/exp/ab.py's two-standard-error rule, beside the sync stage's cost
measured the same way; and whether every call's events equalled the host twin's.

--gate-ends (with --gate-ais, --gate-pocsag or --gate-flex, with or without --gate-bits, or with --gate-route, where it applies to
every route's stage) switches the stage's stretch-end report on, ends the open stretches behind the gate's flush and writes
DIR/ends.jsonl beside the events (under a route: DIR/NAME/ends.jsonl), one line per stretch: channel, first_sample (the stretch's
first input sample, stretch_window * W), outs, mode (0: nothing was being collected when the squelch closed) and the stage's
fields - AIS start_sample and nr_bits of the cut packet; POCSAG baud, nr_words, nr_bits, nr_sync_bits, nr_ok, fail_mask and the
corrected words below nr_ok of the cut batch; FLEX j, eye, coding, fiw, cycle and frame.  With --summary a last line per chain
carries stretches, cut and cut_by_mode.  Without the flag nothing the tool writes changes.

    python tools/level_scan.py --bench-runends [--window 1000] [--reps 8] [--inner 10] [--runends-parent LIB]

prints one JSON line ("run_ends_stage"): the process call of each burst stage at 64 and 1024 channels on the half-open mask, the
report off and on in turn (and the same entry of LIB, another build of the library, as a third variant): means, standard
deviations, on over off with its standard error, and off against LIB by the rule of tools/exp/ab.py.

--gate-route FILE (with --gate-out and --form pcm; not together with --gate-resample, --gate-dc-pole, --gate-bits or a stage flag)
decodes a capture that mixes protocols in one pass: the run router (mfm_runroute_*) stands behind the gate and hands each route's
burst chain only the runs of its own channels.  FILE is JSON:

    {"routes": [{"name": "pocsag", "stage": "pocsag", "resample": "4/5", "taps": "filter.json", "channels": [0, 2, 5]},
                {"name": "flex", "stage": "flex", "resample": "16/25", "taps": "flex.json", "dc_pole": 0.999, "channels": [1, 3]}]}

up to eight routes; stage is ais, pocsag, flex, mm or none (the resampler alone; a route of stage mm carries "mm": {"spb": 20.8333,
"kw": 0.0001, "km": 0.000004, "margin": 0.05}, spb required, as --gate-mm, writes mm.jsonl and chNNNN.mm.s16, takes no bits and has
no stretch-end report, and may carry "sync" as --gate-sync and, with it, "batch" as --gate-batch); resample and taps as --gate-resample and
--resample-taps; dc_pole and bits (true / false) are optional and follow the rules of --gate-dc-pole and --gate-bits (bits only
with ais or pocsag, never with dc_pole); a channel may stand in one route at most, and a channel in none is gated but goes no
further.  Each route runs burst resampler -> stage on its view of the router, on the engine's stream, the flush call included, and
writes under DIR/<name>/ the files the single-stage flags write under DIR, with the same line shapes: resampled.jsonl,
chNNNN.rs.s16, ais.jsonl / pocsag.jsonl / flex.jsonl, pages.jsonl.  Channel numbers stay those of the configuration.
DIR/index.jsonl and DIR/chNNNN.s16 are the gate's, as without the flag.  Two optional keys beside "routes": "shared": true lets a
channel stand in several routes (a carrier that time-shares POCSAG and FLEX reaches both chains), and "pack": true switches
MFM_RUNROUTE_F_PACK on: every route gets a dense payload of its own and its chain is sized to its channels (every route then
needs a channel); the files still carry the configuration's channel numbers.  "local": true (never beside "pack"; every route
needs a channel here too) makes the router with mfm_runroute_create_local: the chains are sized to their routes as under "pack",
but nothing is copied - each route's burst resampler reads the gate's payload in place through its view entries.  The files are
those of "pack", byte for byte.

    python tools/level_scan.py --bench-runroute-local [--window 1000] [--reps 8] [--inner 10]

prints one line ("runroute_local_stage"): the three forms of the router - zero-copy with global channel numbers, packed, local -
on the cases of --bench-runroute-pack, as router + one chain per route (mean, standard deviation and standard error, alternating
in one process in rotating order), local against packed and against zero-copy with the two-standard-error verdict, the three
router calls alone, and the device memory each form takes.

    python tools/level_scan.py --bench-runroute-pack [--window 1000] [--reps 8] [--inner 10] [--pack-only SHAPE/MASK]

prints one line ("runroute_pack_stage"): packed routes against zero-copy routes at 64 and 1024 channels in 2 routes and 1024
channels in 8, the three masks, as router + one chain per route in either form (mean and standard error, alternating in one
process), the two router calls alone (their difference bounds the pack copy from above), the copy's bytes, and the device memory
either form takes.  --pack-only 1024x2/half_open runs one case, for a kernel trace of its own.

    python tools/level_scan.py --bench-runroute [--window 1000] [--reps 8] [--inner 10]

prints one line ("runroute_stage") for the run router at 64 and 1024 channels on idle rows and the three masks all-closed, half-open
and all-open: the router call alone beside the burst resampler's call on an all-closed view, and a two-protocol capture (half the
channels POCSAG at 4/5, half FLEX at 16/25) as router + one chain per route against two whole chains that each read every channel,
alternating in one process in rotating order, with the difference, its standard error and the two-standard-error verdict.

    python tools/level_scan.py --bench [--bench-channels 64] [--form pcm|iq] [--window 4096] [--reps 8] [--gate-preroll 0,1,4]

times the level pass on one 2^26-sample block of the 64- / 1024-channel plan (D = 96, 699 050 outputs per channel)
against the POCSAG stage's call on the same rows (idle input; its slicer, pg_slice_kernel, reads the same bytes) and
against the engine launch with and without filtered IQ.  A line behind it ("level_adaptive_stage"; --bench-level-adaptive prints
that line alone, behind the engine launch that makes the rows) times the level pass with the adaptive squelch off and on (M = 64),
two objects alternating in one process, with the difference, its standard error and the verdict of the same two-standard-error
rule, and the adaptive pass at M = 64, 1 and 1024 (--bench-floor-windows gives other M's; the first is the one set against the
fixed path).  Level pass and comparison alternate in one process, in
rotating order; mean and standard deviation over --reps repetitions, a difference counts beyond two standard errors
(the rule of tools/exp/ab.py).  One JSON line.  A second line times the gate stage on the same rows (whole windows of
them) with every window closed, every window open and the mask a squelch at the median window energy leaves, each beside a
device-to-device copy of the bytes that mask lets through and beside the level pass, alternating in the same process.
With --gate-preroll (one P, or several with commas) there is one such line per P, each with "preroll" and, for P > 0 behind a
P = 0 line of the same run, "gate_ms_over_p0" per mask: the cost of the pre-roll.  The payload of a P > 0 line is what the
dilated mask lets through in the steady state (every call emits the last P windows of the call before it, from the history, and
all but the last P of its own).  With --form pcm a last line ("runrs_stage") times the burst resampler (4/5, 81 taps) behind the
gate for the three masks, alternating in the same process with mfm_resampler_process_device (MFM_RS_FORCE_DOT2) on the full rows:
all-open over that plain resampler as a ratio with its standard error, all-closed as an absolute time.  The line after it
("runrs_dc_stage") times, for the same masks and alternating in the same way, the burst resampler with its DC blocker on (pole
0.999), the burst resampler without it and the plain resampler with dc_block on the full rows: the blocker's cost per mask as a
difference with its standard error, and the burst form over the full-row form as a ratio (--bench-runrs prints these two lines
alone, behind the engine launch that makes the rows).  A line behind it
("runais_stage"; --bench-runais prints that line alone, without the engine) times the burst chain burst resampler -> burst AIS
stage on a gate's device view against the plain chain mfm_resampler -> mfm_ais on the full rows, 4/5 with 41 taps, for the same
three masks and for two row sets of its own: idle (noise) and busy (synthesized AIS frames on every channel).  A last line
("runpocsag_stage"; --bench-runpocsag prints that line alone) does the same for the burst chain burst resampler -> burst POCSAG
stage against mfm_resampler -> mfm_pocsag, busy being synthesized POCSAG transmissions on every channel, and says whether a
sample of the burst events (the first runs of a call) equalled the host twin's.  --bench-runflex prints a line of the same build
("runflex_stage") for the burst chain burst resampler (16/25, 101 taps) -> burst FLEX stage against mfm_resampler -> mfm_flex, busy
being synthesized FLEX frames of the four codings on every channel, the three masks all-closed, half-open (a squelch at the median
window energy) and all-open.  A line after runpocsag_stage ("runbits_stage"; --bench-runbits prints that line alone) is the
A/B of the burst chain's sign-bit path: burst resampler -> burst stage in the PCM form and in the bits form
(mfm_runrs_process_bits_device -> mfm_run{ais,pocsag}_process_bits_device), alternating in one process on one gate call's device
view, for AIS and POCSAG with the ratio, taps and window of their own lines, the busy rows of each and the three masks; per
case the two means and standard deviations, bits over PCM, the difference with its standard error and the verdict of
tools/exp/ab.py's rule (kept / worse beyond two standard errors, else neutral), and whether the two forms' events were identical.

With --gate-bits (only with --gate-ais or --gate-pocsag) the scan routes burst resampler -> burst stage through the bits form:
the same event files; resampled.jsonl keeps its line per run, without file_offset, and no chNNNN.rs.s16 is written, because no
PCM leaves the resampler."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_BPS = 8.0e12  # MI355X HBM3E, spec


def read_config(path):
    cfg = json.load(open(path))
    fs, centre, decim = int(cfg["sampleRateHz"]), int(cfg["centerFreqHz"]), int(cfg["decimationFactor"])
    taps = [float(t) for t in cfg["lpfTaps"]]
    chans = [(int(ch["chanCenterFreq"]), 10.0 ** (float(ch.get("dBGain", 0.0)) / 10.0)) for ch in cfg["channels"]]
    return fs, centre, decim, taps, chans


ROUTE_STAGES = ("ais", "pocsag", "flex", "none")   # and "mm", which the refusal below does not name: its words are pinned
MAX_ROUTES = 8   # MFM_RUNROUTE_MAX_ROUTES
MM_DEFAULTS = {"kw": 0.0001, "km": 0.000004, "margin": 0.05}   # pager/test/test_mueller_muller.c:85-88


def parse_gate_mm(text):
    """--gate-mm SPB[,KW,KM,MARGIN] as the "mm" object of a route"""
    parts = text.split(",")
    if len(parts) not in (1, 4):
        raise SystemExit(f"--gate-mm takes SPB or SPB,KW,KM,MARGIN, not {text!r}")
    try:
        vals = [float(x) for x in parts]
    except ValueError:
        raise SystemExit(f"--gate-mm takes SPB or SPB,KW,KM,MARGIN, not {text!r}")
    mm = dict(MM_DEFAULTS, spb=vals[0])
    if len(vals) == 4:
        mm.update(kw=vals[1], km=vals[2], margin=vals[3])
    return mm


def check_mm(mm, where):
    """the "mm" object of a route (or of --gate-mm): spb, and optionally kw, km, margin, all numbers"""
    if not isinstance(mm, dict) or "spb" not in mm or set(mm) - {"spb", "kw", "km", "margin"} or \
            not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in mm.values()):
        raise SystemExit(f"{where}: \"mm\" must be an object of numbers with spb and optionally kw, km and margin, not {mm!r}")
    return dict(MM_DEFAULTS, **mm)


def parse_gate_sync(text):
    """--gate-sync WORD[,WORD...][/DIST][,either] as the "sync" object of a route of stage mm"""
    either = text.endswith(",either")
    body = text[:-len(",either")] if either else text
    words, _, dist = body.partition("/")
    try:
        sync = {"words": [int(w, 0) for w in words.split(",")], "distance": int(dist) if dist else 3, "either": either}
    except ValueError:
        raise SystemExit(f"--gate-sync takes WORD[,WORD...][/DIST][,either], not {text!r}")
    return check_sync(sync, "--gate-sync")


def check_sync(sync, where):
    """the "sync" object of a route of stage mm (or of --gate-sync): words, 1 .. 8 of 32 bits, and optionally distance (0 .. 15) and
    either"""
    ok = isinstance(sync, dict) and "words" in sync and not set(sync) - {"words", "distance", "either"}
    ok = ok and isinstance(sync["words"], list) and 1 <= len(sync["words"]) <= 8
    ok = ok and all(isinstance(w, int) and not isinstance(w, bool) and 0 <= w <= 0xFFFFFFFF for w in sync["words"])
    ok = ok and isinstance(sync.get("distance", 3), int) and 0 <= sync.get("distance", 3) <= 15 and isinstance(sync.get("either", False), bool)
    if not ok:
        raise SystemExit(f"{where}: \"sync\" must be an object with words (1 .. 8 numbers of 32 bits) and optionally distance (0 .. 15) "
                         f"and either (true or false), not {sync!r}")
    return {"words": list(sync["words"]), "distance": sync.get("distance", 3), "either": sync.get("either", False)}


def parse_gate_batch(text):
    """--gate-batch [KEEP[,BAUD]] as the "batch" object of a route of stage mm"""
    keep, _, baud = text.partition(",")
    try:
        batch = {"keep": int(keep) if keep else 4, "baud": int(baud) if baud else 1200}
    except ValueError:
        raise SystemExit(f"--gate-batch takes [KEEP[,BAUD]], not {text!r}")
    return check_batch(batch, "--gate-batch")


def check_batch(batch, where):
    """the "batch" object of a route of stage mm (or of --gate-batch): optionally keep (0 .. 15) and baud (1 .. 65535, what the
    pages carry)"""
    ok = isinstance(batch, dict) and not set(batch) - {"keep", "baud"}
    ok = ok and all(isinstance(v, int) and not isinstance(v, bool) for v in batch.values())
    ok = ok and 0 <= batch.get("keep", 4) <= 15 and 1 <= batch.get("baud", 1200) <= 65535
    if not ok:
        raise SystemExit(f"{where}: \"batch\" must be an object with optionally keep (0 .. 15) and baud (1 .. 65535), not {batch!r}")
    return {"keep": batch.get("keep", 4), "baud": batch.get("baud", 1200)}


class Routes(list):
    """the routes of a --gate-route file; `local` is the file's "local" key"""
    local = False


def read_routes(path, nr_channels):
    """--gate-route FILE: {"routes": [{"name", "stage", "resample", "taps", "channels", and optionally "dc_pole", "bits"}], and
    optionally "shared": true (a channel may stand in several routes), "pack": true (MFM_RUNROUTE_F_PACK: every route's chain
    is sized to its channels) and "local": true (mfm_runroute_create_local: sized likewise, on the gate's payload in place; not
    beside "pack")}, checked; what is wrong ends the run with a message.  Returns (routes, shared, pack); routes.local is the
    third key"""
    doc = json.load(open(path))
    routes = Routes(doc["routes"])
    shared, pack, local = doc.get("shared", False), doc.get("pack", False), doc.get("local", False)
    for key, value in (("shared", shared), ("pack", pack), ("local", local)):
        if not isinstance(value, bool):
            raise SystemExit(f"--gate-route: \"{key}\" must be true or false, not {value!r}")
    if local and pack:
        raise SystemExit("--gate-route: \"local\" and \"pack\" exclude each other: both size every route's chain to its channels, "
                         "\"pack\" on a copy of the route's windows and \"local\" on the gate's payload in place")
    routes.local = local
    if not 1 <= len(routes) <= MAX_ROUTES:
        raise SystemExit(f"--gate-route: {len(routes)} routes; the run router takes 1 .. {MAX_ROUTES}")
    names, owner = set(), {}
    for r in routes:
        name = r.get("name", "")
        if not name or name in names or os.sep in name or name in (".", ".."):
            raise SystemExit(f"--gate-route: a route's name is its folder under --gate-out: {name!r} is empty, used twice or a path")
        names.add(name)
        if r.get("stage") not in ROUTE_STAGES + ("mm",):
            raise SystemExit(f"--gate-route: route {name}: stage {r.get('stage')!r} is none of {', '.join(ROUTE_STAGES)}")
        if not r.get("resample") or not r.get("taps"):
            raise SystemExit(f"--gate-route: route {name} needs resample (I/D) and taps (a JSON file whose lpfCoeffs are the taps)")
        if r["stage"] == "mm":
            r["mm"] = check_mm(r.get("mm"), f"--gate-route: route {name}")
            if "sync" in r:
                r["sync"] = check_sync(r["sync"], f"--gate-route: route {name}")
            if "batch" in r:
                if "sync" not in r:
                    raise SystemExit(f"--gate-route: route {name}: \"batch\" needs \"sync\": the burst batch stage takes the burst sync "
                                     "stage's events and bits")
                r["batch"] = check_batch(r["batch"], f"--gate-route: route {name}")
            if r.get("bits"):
                raise SystemExit(f"--gate-route: route {name}: bits needs stage ais or pocsag: the burst Mueller-Muller stage reads PCM values, "
                                 "not sign bits")
        elif "mm" in r:
            raise SystemExit(f"--gate-route: route {name}: \"mm\" belongs to stage mm, not to stage {r['stage']}")
        elif "sync" in r:
            raise SystemExit(f"--gate-route: route {name}: \"sync\" belongs to stage mm, not to stage {r['stage']}")
        elif "batch" in r:
            raise SystemExit(f"--gate-route: route {name}: \"batch\" belongs to stage mm, not to stage {r['stage']}")
        if r.get("bits") and r["stage"] not in ("ais", "pocsag"):
            raise SystemExit(f"--gate-route: route {name}: bits needs stage ais or pocsag: the burst FLEX stage reads PCM values, not sign bits")
        if r.get("bits") and r.get("dc_pole") is not None:
            raise SystemExit(f"--gate-route: route {name}: dc_pole and bits exclude each other: the DC blocker filters the PCM the sign "
                             "bits would be taken from")
        for c in r.get("channels", []):
            if not isinstance(c, int) or not 0 <= c < nr_channels:
                raise SystemExit(f"--gate-route: route {name}: channel {c!r} is not one of the configuration's {nr_channels}")
            if c in owner and (not shared or owner[c] == name):
                raise SystemExit(f"--gate-route: channel {c} is in two routes ({owner[c]} and {name}): a channel has one route")
            owner[c] = name
        r["channels"] = list(r.get("channels", []))
        if (pack or local) and not r["channels"]:
            raise SystemExit(f"--gate-route: route {name} has no channel: with \"{'pack' if pack else 'local'}\" every route's chain is "
                             "sized to its channels")
    return routes, shared, pack


# --gate-ends: the fields of a stretch-end record a line of ends.jsonl carries beside channel, first_sample, outs and mode
ENDS_LINE_FIELDS = {"ais": ("start_sample", "nr_bits"), "pocsag": ("baud", "nr_words", "nr_bits", "nr_sync_bits", "nr_ok", "fail_mask"),
                    "flex": ("j", "eye", "coding", "fiw", "cycle", "frame")}
ENDS_MODE_NAMES = {"ais": {1: "receive"}, "pocsag": {2: "batch", 3: "syncword"}, "flex": {1: "sync1", 2: "frame"}}


class BurstChain:
    """burst resampler -> burst stage (ais, pocsag, flex, mm or None) behind one run list - the gate's, or with --gate-route one
    route's of the run router - and the files the two write under out_dir; view() returns the run list's device view"""

    def __init__(self, pkg, out_dir, window, nr_channels, max_in_samples, preroll, device, view, resample, taps_file, dc_pole=None,
                 stage=None, bits=False, caps=None, channels=None, bound=None, ends=False, mm=None, sync=None, batch=None):
        """caps and channels: behind a packed or a local route of the run router, its route_caps() - the chain is sized to the route -
        and its route_channels(), which turn the route-local channel numbers of everything fetched back into true ones.  bound:
        behind a local route, the router's bound_view(): the resampler then reads the gate's payload through its view entries.
        ends (--gate-ends): the stage's stretch-end report, one line per stretch in ends.jsonl (the mm stage has none: nothing is
        pending when a stretch ends).  mm: stage mm's spb, kw, km and margin.  sync (--gate-sync): the burst sync stage behind
        stage mm, its words, distance and either.  batch (--gate-batch): the burst batch stage behind the sync stage, its keep
        distance and the baud rate its pages carry"""
        b = self.b = pkg.binding
        self.out_dir, self.window, self.view, self.bound = out_dir, window, view, bound
        self.channels = None if channels is None else np.asarray(channels, np.uint32)
        interp, decim_rs = [int(x) for x in resample.split("/")]
        co = np.array([int(float(t) * 16384.0) for t in json.load(open(taps_file))["lpfCoeffs"]], np.int16)  # decoder.c:530-533
        if caps is not None:
            nr_channels, max_windows, max_runs = caps
            self.rr = pkg.RunResampler(nr_channels, co, interp, decim_rs, window, max_in_samples=max_in_samples, preroll_windows=preroll,
                                       max_windows=max_windows, max_runs=max_runs, device=device)
        else:
            self.rr = pkg.RunResampler(nr_channels, co, interp, decim_rs, window, max_in_samples=max_in_samples, preroll_windows=preroll,
                                       device=device)
        if dc_pole is not None:
            self.rr.set_dc_block(dc_pole)
        self.rs_index, self.rs_started = open(os.path.join(out_dir, "resampled.jsonl"), "w"), set()
        self.stage = stage
        self.st, self.st_index, self.pages_index, self.pagers = None, None, None, {}
        if stage == "mm":
            self.st = pkg.RunMm.behind(self.rr, mm["spb"], mm["kw"], mm["km"], margin=mm["margin"], device=device)
            self.st_index, self.mm_started = open(os.path.join(out_dir, "mm.jsonl"), "w"), set()
        elif stage:
            self.st = {"ais": pkg.RunAis, "pocsag": pkg.RunPocsag, "flex": pkg.RunFlex}[stage].behind(self.rr, device=device)
            self.st_index = open(os.path.join(out_dir, stage + ".jsonl"), "w")
        self.sy, self.sy_index, self.sy_words, self.sy_stretch = None, None, [], {}
        if stage == "mm" and sync:
            self.sy = pkg.RunSync.behind(self.st, sync["words"], max_distance=sync["distance"], either=sync["either"], device=device)
            self.sy_index, self.sy_words = open(os.path.join(out_dir, "sync.jsonl"), "w"), ["%08x" % w for w in sync["words"]]
        self.bt, self.bt_index, self.bt_baud = None, None, 0
        if self.sy and batch:
            self.bt = pkg.RunBatch.behind(self.sy, keep_distance=batch["keep"], device=device)
            self.bt_index, self.bt_baud = open(os.path.join(out_dir, "batch.jsonl"), "w"), batch["baud"]
        if stage in ("pocsag", "flex") or self.bt:
            self.pages_index = open(os.path.join(out_dir, "pages.jsonl"), "w")
        self.ends_index, self.stretches, self.cut_by_mode = None, 0, {}
        if stage and stage != "mm" and ends:
            self.st.set_end_report(True)
            self.ends_index = open(os.path.join(out_dir, "ends.jsonl"), "w")
        # --gate-bits: the predicate the stage behind the resampler reads
        self.bits_polarity = (b.MFM_BITS_POS if stage == "ais" else b.MFM_BITS_NEG) if bits else 0

    def run(self, stream):
        """burst resampler and the stage behind it on the run list's last result"""
        rr, st = self.rr, self.st
        if self.bits_polarity:
            if self.bound is not None:
                rr.process_bits_view_device(*self.view(), self.bound, self.bits_polarity, stream=stream)
            else:
                rr.process_bits_device(*self.view(), self.bits_polarity, stream=stream)
            st.process_bits_device(rr.bits_view(), stream=stream)
            return
        if self.bound is not None:
            rr.process_view_device(*self.view(), self.bound, stream=stream)
        else:
            rr.process_device(*self.view(), stream=stream)
        if st:
            st.process_device(*rr.device_view(), stream=stream)
        if self.sy:
            self.sy.process_device(*st.device_view(), stream=stream)
        if self.bt:
            self.bt.process_device(*self.sy.device_view(), stream=stream)

    def write(self):
        """fetch the last call's results and append them to the files"""
        if self.bits_polarity:
            self.write_resampled_runs(self.true_channels(self.rr.fetch_bits()[0]))
        else:
            runs, payload = self.rr.fetch()
            self.write_resampled(self.true_channels(runs), payload)
        if self.stage == "ais":
            self.write_ais(self.true_channels(self.st.fetch()))
        if self.stage == "pocsag":
            self.write_pocsag(self.true_channels(self.st.fetch()))
        if self.stage == "flex":
            events, frames = self.st.fetch()
            self.write_flex(self.true_channels(events), frames)
        if self.stage == "mm":
            runs, decisions = self.st.fetch()
            self.write_mm(self.true_channels(runs), decisions)
        if self.sy:
            runs, _, events = self.sy.fetch()
            self.write_sync(self.true_channels(runs), self.true_channels(events))
        if self.bt:
            self.write_batch(self.true_channels(self.bt.fetch()))
        if self.ends_index:
            self.write_ends(self.true_channels(self.st.fetch_ends()))

    def end(self, stream):
        """--gate-ends, behind the gate's flush: the stretches still open end here"""
        if self.ends_index:
            self.st.end_stretches(stream=stream)
            self.write_ends(self.true_channels(self.st.fetch_ends()))

    def write_ends(self, ends):
        """one line per stretch: where it began in the input, how many outputs it had, what state it ended in"""
        for e in ends:
            line = {"channel": int(e["channel"]), "first_sample": int(e["stretch_window"]) * self.window, "outs": int(e["outs"]),
                    "mode": int(e["mode"])}
            line.update({f: int(e[f]) for f in ENDS_LINE_FIELDS[self.stage]})
            if self.stage == "pocsag":   # the whole codewords of the batch the squelch cut, as far as the BCH accepted them
                line["corrected"] = ["%08x" % int(w) for w in e["corrected"][:int(e["nr_ok"])]]
            self.ends_index.write(json.dumps(line) + "\n")
            self.stretches += 1
            if line["mode"]:
                self.cut_by_mode[ENDS_MODE_NAMES[self.stage][line["mode"]]] = self.cut_by_mode.get(ENDS_MODE_NAMES[self.stage][line["mode"]], 0) + 1

    def ends_summary(self):
        return {"stretches": self.stretches, "cut": sum(self.cut_by_mode.values()), "cut_by_mode": dict(sorted(self.cut_by_mode.items()))}

    def true_channels(self, records):
        """behind a packed or a local route: the records with their route-local channel numbers mapped back, before anything is written"""
        if self.channels is not None and len(records):
            records = records.copy()
            records["channel"] = self.channels[records["channel"]]
        return records

    def close(self):
        for hp in self.pagers.values():
            hp.close()
        if self.sy:
            for c in sorted(self.sy_stretch):
                self.write_sync_summary(c)
            self.sy_index.close()
        if self.bt:
            self.bt_index.close()
            self.bt.close()
        if self.sy:
            self.sy.close()
        for f in (self.rs_index, self.st_index, self.pages_index, self.ends_index):
            if f:
                f.close()
        if self.st:
            self.st.close()
        self.rr.close()

    def write_flex(self, events, frames):
        """the events, and the messages of a fresh host FLEX pager per (channel, stretch)"""
        b, pagers = self.b, self.pagers
        for e in events:
            c, first = int(e["channel"]), int(e["stretch_window"]) * self.window
            line = {"channel": c, "first_sample": first}
            line.update({f: int(e[f]) for f in FLEX_LINE_FIELDS})
            self.st_index.write(json.dumps(line) + "\n")
            if c not in pagers or pagers[c].first != first:
                if c in pagers:
                    pagers[c].close()
                pagers[c] = HostFlexPager(c, first, self.pages_index)
            pagers[c].on_events(b.runflex_to_flex_events(np.array([e], b.RUNFLEX_EVENT_DTYPE)), frames)

    def write_pocsag(self, events):
        """the events, and the pages of a fresh host pager per (channel, stretch)"""
        b, pagers = self.b, self.pagers
        for e in events:
            c, first = int(e["channel"]), int(e["stretch_window"]) * self.window
            self.st_index.write(json.dumps({"channel": c, "first_sample": first, "type": int(e["type"]), "baud": int(e["baud"]),
                                            "sample": int(e["sample"]), "aux": int(e["aux"]), "nr_ok": int(e["nr_ok"]),
                                            "fail_mask": int(e["fail_mask"]),
                                            "corrected": ["%08x" % int(w) for w in e["corrected"]] if int(e["type"]) == 2 else []}) + "\n")
            if c not in pagers or pagers[c].first != first:
                if c in pagers:
                    pagers[c].close()
                pagers[c] = HostPager(c, first, self.pages_index)
            pagers[c].on_events(b.runpocsag_to_pocsag_events(np.array([e], b.RUNPOCSAG_EVENT_DTYPE)))

    def write_ais(self, events):
        for e in events:
            self.st_index.write(json.dumps({"channel": int(e["channel"]), "first_sample": int(e["stretch_window"]) * self.window,
                                            "sample": int(e["sample"]), "start_sample": int(e["start_sample"]), "nr_bytes": int(e["nr_bytes"]),
                                            "fcs_valid": int(e["fcs_valid"]), "bytes": bytes(e["bytes"][:int(e["nr_bytes"])]).hex()}) + "\n")

    def write_mm(self, runs, decisions):
        """the decisions of every run appended to its channel's file, and a line per run"""
        for r in runs:
            c = int(r["channel"])
            path = os.path.join(self.out_dir, "ch%04d.mm.s16" % c)
            with open(path, "ab" if c in self.mm_started else "wb") as g:
                at = g.tell()
                decisions[int(r["dec_offset"]):int(r["dec_offset"]) + int(r["nr_dec"])].tofile(g)
            self.mm_started.add(c)
            self.st_index.write(json.dumps({"channel": c, "first_sample": int(r["first_window"]) * self.window,
                                            "first_dec": int(r["first_dec"]), "nr_dec": int(r["nr_dec"]), "begins": int(r["flags"]) & 1,
                                            "file_offset": at}) + "\n")

    def write_sync(self, runs, events):
        """a line per event, and a summary line per stretch once the channel's next stretch begins (or the run ends)"""
        at = 0
        for r in runs:
            c = int(r["channel"])
            if int(r["flags"]) & 1:
                if c in self.sy_stretch:
                    self.write_sync_summary(c)
                self.sy_stretch[c] = [int(r["first_window"]), 0, [0] * len(self.sy_words)]
            st = self.sy_stretch[c]
            st[1] += int(r["nr_dec"])
            for e in events[at:at + int(r["nr_events"])]:
                k = int(e["word_index"])
                st[2][k] += 1
                self.sy_index.write(json.dumps({"channel": c, "first_window": st[0], "first_sample": st[0] * self.window, "dec": int(e["dec"]),
                                                "word": self.sy_words[k], "distance": int(e["distance"]), "inverted": int(e["inverted"]),
                                                "seen": "%08x" % int(e["seen"])}) + "\n")
            at += int(r["nr_events"])

    def write_batch(self, events):
        """a line per event, and the pages of a fresh host pager per (channel, stretch)"""
        b, pagers = self.b, self.pagers
        for e in events:
            c, fw = int(e["channel"]), int(e["stretch_window"])
            first = fw * self.window
            line = {"channel": c, "first_window": fw, "first_sample": first, "type": int(e["type"]), "dec": int(e["dec"]),
                    "aux": "%08x" % int(e["aux"]), "word": self.sy_words[int(e["word_index"])], "inverted": int(e["inverted"]),
                    "nr_ok": int(e["nr_ok"]), "fail_mask": int(e["fail_mask"])}
            if int(e["type"]) == 2:
                line["corrected"] = ["%08x" % int(w) for w in e["corrected"]]
            self.bt_index.write(json.dumps(line) + "\n")
            if c not in pagers or pagers[c].first != first:
                if c in pagers:
                    pagers[c].close()
                pagers[c] = HostPager(c, first, self.pages_index)
            pagers[c].on_events(b.runbatch_to_pocsag_events(np.array([e], b.RUNBATCH_EVENT_DTYPE), self.bt_baud))

    def write_sync_summary(self, c):
        fw, nd, counts = self.sy_stretch.pop(c)
        self.sy_index.write(json.dumps({"channel": c, "first_window": fw, "first_sample": fw * self.window, "decisions": nd,
                                        "events": dict(zip(self.sy_words, counts))}) + "\n")

    def write_resampled(self, runs, payload):
        for r in runs:
            c = int(r["channel"])
            path = os.path.join(self.out_dir, "ch%04d.rs.s16" % c)
            with open(path, "ab" if c in self.rs_started else "wb") as g:
                at = g.tell()
                payload[int(r["out_offset"]):int(r["out_offset"]) + int(r["nr_out"])].tofile(g)
            self.rs_started.add(c)
            self.rs_index.write(json.dumps({"channel": c, "first_sample": int(r["first_window"]) * self.window,
                                            "first_out": int(r["first_out"]), "nr_out": int(r["nr_out"]), "begins": int(r["flags"]) & 1,
                                            "file_offset": at}) + "\n")

    def write_resampled_runs(self, runs):
        """the bits form: the runs alone, no PCM left the resampler"""
        for r in runs:
            self.rs_index.write(json.dumps({"channel": int(r["channel"]), "first_sample": int(r["first_window"]) * self.window,
                                            "first_out": int(r["first_out"]), "nr_out": int(r["nr_out"]), "begins": int(r["flags"]) & 1}) + "\n")


def scan(a):
    import torch  # noqa: F401  (brings the HIP runtime up before the library does)
    from __graft_entry__ import load_package
    pkg = load_package()
    b = pkg.binding
    fs, centre, decim, taps, chans = read_config(a.config)
    routes, shared, pack = read_routes(a.gate_route, len(chans)) if a.gate_route else (None, False, False)
    local = routes is not None and routes.local
    iq_form = a.form == "iq"
    sense = a.sense or ("above" if iq_form else "below")
    adaptive = a.floor_windows is not None
    if adaptive and sense == "below" and a.open_thr == 0 and a.close_thr is None:
        a.open_thr = (1 << 64) - 1   # no absolute limit on the low side
    eng = pkg.Engine(fs, decim, a.block, device=a.device, flags=b.MFM_F_DEVICE_ONLY)
    for freq, gain in chans:
        eng.add_channel(freq - centre, taps, gain, want_iq=iq_form)
    eng.commit()
    lv = pkg.Level(len(chans), a.block // decim + 8, a.window, form=b.MFM_LEVEL_IQ if iq_form else b.MFM_LEVEL_PCM,
                   metric=b.MFM_LEVEL_METRIC_DIFF if a.metric == "diff" else b.MFM_LEVEL_METRIC_ENERGY,
                   sense=b.MFM_LEVEL_OPEN_ABOVE if sense == "above" else b.MFM_LEVEL_OPEN_BELOW,
                   open_thr=a.open_thr, close_thr=a.close_thr if a.close_thr is not None else a.open_thr, hang_windows=a.hang,
                   device=a.device)
    if adaptive:
        lv.set_adaptive(a.floor_windows, int(round(256.0 * a.open_ratio)), int(round(256.0 * a.close_ratio)), a.warmup or 0)
    gate, index, started = None, None, set()
    elems = 2 if iq_form else 1
    if a.gate_out:
        os.makedirs(a.gate_out, exist_ok=True)
        gate = pkg.Gate(len(chans), a.block // decim + 8, a.window, elems_per_sample=elems, device=a.device,
                        preroll_windows=int(a.gate_preroll))
        index = open(os.path.join(a.gate_out, "index.jsonl"), "w")
    if a.gate_resample and (not gate or iq_form):
        raise SystemExit("--gate-resample needs --gate-out and --form pcm: the burst resampler takes PCM payloads only")
    if a.gate_resample and not a.resample_taps:
        raise SystemExit("--gate-resample needs --resample-taps FILE")
    if a.gate_ais and not a.gate_resample:
        raise SystemExit("--gate-ais needs --gate-resample: the burst AIS stage takes the burst resampler's runs")
    if a.gate_pocsag and not a.gate_resample:
        raise SystemExit("--gate-pocsag needs --gate-resample: the burst POCSAG stage takes the burst resampler's runs")
    if a.gate_pocsag and a.gate_ais:
        raise SystemExit("--gate-pocsag and --gate-ais exclude each other: one stage reads the burst resampler's runs")
    max_in = a.block // decim + 8
    router, chains = None, []   # one chain behind the gate, or with --gate-route one per route behind the run router
    if a.gate_resample:   # main() has refused --gate-flex without it or beside another stage
        stage = "ais" if a.gate_ais else "pocsag" if a.gate_pocsag else "flex" if a.gate_flex else "mm" if a.gate_mm else None
        chains.append(BurstChain(pkg, a.gate_out, a.window, len(chans), max_in, int(a.gate_preroll), a.device, gate.device_view,
                                 a.gate_resample, a.resample_taps, dc_pole=a.gate_dc_pole, stage=stage, bits=a.gate_bits, ends=a.gate_ends,
                                 mm=parse_gate_mm(a.gate_mm) if a.gate_mm else None,
                                 sync=parse_gate_sync(a.gate_sync) if a.gate_sync else None,
                                 batch=parse_gate_batch(a.gate_batch) if a.gate_batch is not None else None))
    if routes is not None:
        if not gate or iq_form:
            raise SystemExit("--gate-route needs --gate-out and --form pcm: the burst resamplers take PCM payloads only")
        if shared or pack or local:   # a set of routes per channel
            table = np.zeros(len(chans), np.uint8)
            for k, r in enumerate(routes):
                table[r["channels"]] |= 1 << k
            router = pkg.RunRouter.behind(None, len(routes), max_in, a.window, preroll_windows=int(a.gate_preroll), device=a.device,
                                          sets=table, pack=pack, local=local)
        else:
            table = np.full(len(chans), b.MFM_ROUTE_NONE, np.uint8)
            for k, r in enumerate(routes):
                table[r["channels"]] = k
            router = pkg.RunRouter.behind(table, len(routes), max_in, a.window, preroll_windows=int(a.gate_preroll), device=a.device)
        for k, r in enumerate(routes):
            os.makedirs(os.path.join(a.gate_out, r["name"]), exist_ok=True)
            sized = dict(caps=router.route_caps(k), channels=router.route_channels(k)) if pack or local else {}
            if local:
                sized["bound"] = router.bound_view()
            chains.append(BurstChain(pkg, os.path.join(a.gate_out, r["name"]), a.window, len(chans), max_in, int(a.gate_preroll), a.device,
                                     lambda k=k: router.device_view(k), r["resample"], r["taps"], dc_pole=r.get("dc_pole"),
                                     stage=None if r["stage"] == "none" else r["stage"], bits=bool(r.get("bits")), ends=a.gate_ends,
                                     mm=r.get("mm"), sync=r.get("sync"), batch=r.get("batch"), **sized))

    def run_stages():
        """the router, where there is one, and every chain on the gate's last result, all on the engine's stream"""
        if router:
            router.process_device(*gate.device_view(), stream=eng.stream)
        for ch in chains:
            ch.run(eng.stream)

    def write_runs(runs, payload):
        for r in runs:
            c, n_el = int(r["channel"]), int(r["nr_windows"]) * a.window * elems
            path = os.path.join(a.gate_out, "ch%04d.s16" % c)
            with open(path, "ab" if c in started else "wb") as g:
                at = g.tell()
                payload[int(r["payload_offset"]):int(r["payload_offset"]) + n_el].tofile(g)
            started.add(c)
            index.write(json.dumps({"channel": c, "first_sample": int(r["first_window"]) * a.window,
                                    "nr_samples": int(r["nr_windows"]) * a.window, "file_offset": at}) + "\n")

    fmt = {"cs16": b.MFM_IN_CS16, "cs8": b.MFM_IN_CS8, "cu8": b.MFM_IN_CU8}[a.format]
    bytes_per_sample = 4 if a.format == "cs16" else 2
    windows = np.zeros(len(chans), np.int64)
    opened = np.zeros(len(chans), np.int64)
    floors = [[] for _ in chans]
    out = sys.stdout
    with open(a.input, "rb") as f:
        while True:
            raw = f.read(a.block * bytes_per_sample)
            n = len(raw) // bytes_per_sample
            if n == 0:
                break
            data = np.frombuffer(raw[:n * bytes_per_sample], np.int16 if a.format == "cs16" else np.uint8)
            rc = eng.push_bytes(data, fmt)
            if rc < 0:
                raise pkg.MfmError(rc, "mfm_engine_push_bytes", eng.lib.mfm_last_error().decode())
            d_pcm, stride, nout, d_iq = eng.last_output_device()
            if iq_form:
                lv.process_device(d_iq, 2 * stride, nout, stream=eng.stream)
            else:
                lv.process_device(d_pcm, stride, nout, stream=eng.stream)
            if gate:
                d_rec, rec_stride, nw, _ = lv.device_view()
                rows = (d_iq, 2 * stride) if iq_form else (d_pcm, stride)
                gate.process_device(rows[0], rows[1], nout, d_rec, rec_stride, nw, stream=eng.stream)
                run_stages()
            rec = lv.fetch()
            fl = lv.fetch_floor() if adaptive else None
            if gate:
                write_runs(*gate.fetch())
            for ch in chains:
                ch.write()
            for c, (freq, _) in enumerate(chans):
                for i, r in enumerate(rec[c]):
                    line = {"freq": freq, "channel": c, "window": int(r["window"]), "energy": int(r["energy"]),
                            "diff_energy": int(r["diff_energy"]), "peak": int(r["peak"]), "open": int(r["open"])}
                    if adaptive:
                        line["floor"] = int(fl[c, i])
                        floors[c].append(int(fl[c, i]))
                    out.write(json.dumps(line) + "\n")
            windows += rec.shape[1]
            opened += rec["open"].sum(axis=1).astype(np.int64)
    if a.summary:
        for c, (freq, _) in enumerate(chans):
            line = {"summary": True, "freq": freq, "channel": c, "windows": int(windows[c]), "open_windows": int(opened[c]),
                    "open_share": (float(opened[c]) / float(windows[c])) if windows[c] else 0.0}
            if adaptive:
                line["median_floor"] = sorted(floors[c])[(len(floors[c]) - 1) // 2] if floors[c] else 0
            out.write(json.dumps(line) + "\n")
    if gate:
        gate.flush_device(stream=eng.stream)  # the windows pre-roll still held back; none with P = 0
        run_stages()
        write_runs(*gate.fetch())
        for k, ch in enumerate(chains):
            ch.write()
            ch.end(eng.stream)
            if a.summary and ch.ends_index:
                line = {"summary": True, "ends": True}
                if routes is not None:
                    line["route"] = routes[k]["name"]
                line.update(ch.ends_summary())
                out.write(json.dumps(line) + "\n")
            ch.close()
        if router:
            router.close()
        index.close()
        gate.close()
    lv.close()
    eng.close()


class HostPager:
    """host/mfm_pager_pocsag.c through libmfm_host.so: one pager for one stretch of one channel; every page goes to `out` as a
    JSON line in the shape decoder_amd prints (decoder_main.c on_page), the channel and the stretch in the place of the time"""
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint16, C.c_uint32, C.POINTER(C.c_char), C.c_size_t, C.c_uint8)

    def __init__(self, channel, first, out):
        so = os.path.join(ROOT, "tsl-sdr_amd", "host", "libmfm_host.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run make -C tsl-sdr_amd")
        self.h = C.CDLL(so)
        self.channel, self.first, self.out = channel, first, out
        self._num = self.CB(lambda p, baud, cap, data, n, fn: self._page("numeric", baud, cap, data, n, fn))
        self._alpha = self.CB(lambda p, baud, cap, data, n, fn: self._page("alphanumeric", baud, cap, data, n, fn))
        self.p = C.c_void_p()
        self.h.pager_pocsag_new.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, self.CB, self.CB, C.c_bool]
        self.h.pager_pocsag_on_events.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.h.pager_pocsag_delete.argtypes = [C.POINTER(C.c_void_p)]
        if self.h.pager_pocsag_new(C.byref(self.p), 0, self._num, self._alpha, False) != 0:
            raise SystemExit("pager_pocsag_new failed")

    def _page(self, kind, baud, cap, data, n, fn):
        text = "".join({3: " ", 4: " ", 0x17: " ", 8: "<BKSP>", 12: "<FF>"}.get(ch, chr(ch)) for ch in C.string_at(data, n))
        self.out.write(json.dumps({"proto": "pocsag", "type": kind, "channel": self.channel, "first_sample": self.first, "baud": int(baud),
                                   "capCode": int(cap), "function": int(fn), "message": text}) + "\n")
        return 0

    def on_events(self, ev):
        ev = np.ascontiguousarray(ev)
        if self.h.pager_pocsag_on_events(self.p, ev.ctypes.data, ev.size) != 0:
            raise SystemExit("pager_pocsag_on_events failed")

    def close(self):
        self.h.pager_pocsag_delete(C.byref(self.p))


FLEX_LINE_FIELDS = ("type", "sample", "sync_sample", "coding", "baud", "eye", "a", "b", "inv_a", "fiw_raw", "fiw", "fiw_rc", "sample_range",
                    "sample_delta", "cycle", "frame", "nr_phases")


class HostFlexPager:
    """host/mfm_pager_flex.c through libmfm_host.so: one pager for one stretch of one channel; every message goes to `out` as a
    JSON line in the shape decoder_amd prints (decoder_main.c), the channel and the stretch in the place of the time"""
    ALN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint16, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint64, C.c_bool, C.c_bool, C.c_uint8,
                      C.POINTER(C.c_char), C.c_size_t)
    NUM = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint16, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint64, C.POINTER(C.c_char), C.c_size_t)
    SIV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint16, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint64, C.c_uint8, C.c_uint32)

    def __init__(self, channel, first, out):
        so = os.path.join(ROOT, "tsl-sdr_amd", "host", "libmfm_host.so")
        if not os.path.exists(so):
            raise SystemExit(f"{so} missing: run make -C tsl-sdr_amd")
        self.h = C.CDLL(so)
        self.channel, self.first, self.out = channel, first, out
        self._aln = self.ALN(lambda f, baud, ph, cy, fr, cap, frag, md, seq, data, n: self._line(
            "alphanumeric", baud, ph, cy, fr, cap, fragment=bool(frag), maildrop=bool(md), fragSeq=int(seq), message=self._text(data, n)))
        self._num = self.NUM(lambda f, baud, ph, cy, fr, cap, data, n: self._line("numeric", baud, ph, cy, fr, cap, message=self._text(data, n)))
        self._siv = self.SIV(lambda f, baud, ph, cy, fr, cap, t, d: self._line(
            "tempAddrActivation", baud, ph, cy, fr, cap, startFrameNo=int(d) & 0x7F, tempAddressId=(int(d) >> 7) & 0xF) if t == 0 else 0)
        self.p = C.c_void_p()
        self.h.pager_flex_new.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, self.ALN, self.NUM, self.SIV]
        self.h.pager_flex_on_events.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        self.h.pager_flex_delete.argtypes = [C.POINTER(C.c_void_p)]
        if self.h.pager_flex_new(C.byref(self.p), 0, self._aln, self._num, self._siv) != 0:
            raise SystemExit("pager_flex_new failed")

    @staticmethod
    def _text(data, n):
        return "".join({3: " ", 4: " ", 0x17: " ", 8: "<BKSP>", 12: "<FF>"}.get(ch, chr(ch)) for ch in C.string_at(data, n))

    def _line(self, kind, baud, phase, cycle, frame, cap, **rest):
        line = {"proto": "flex", "type": kind, "channel": self.channel, "first_sample": self.first, "baud": int(baud), "frameNo": int(frame),
                "cycleNo": int(cycle), "phaseNo": "ABCD"[int(phase)], "capCode": int(cap)}
        line.update(rest)
        self.out.write(json.dumps(line) + "\n")
        return 0

    def on_events(self, ev, frames):
        ev, frames = np.ascontiguousarray(ev), np.ascontiguousarray(frames)
        if self.h.pager_flex_on_events(self.p, ev.ctypes.data, ev.size, frames.ctypes.data) != 0:
            raise SystemExit("pager_flex_on_events failed")

    def close(self):
        self.h.pager_flex_delete(C.byref(self.p))


def _stats(xs):
    m = sum(xs) / len(xs)
    sd = math.sqrt(sum((x - m) ** 2 for x in xs) / (len(xs) - 1)) if len(xs) > 1 else float("nan")
    return m, sd


def bench(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    b = pkg.binding
    if not torch.cuda.is_available():
        raise SystemExit("--bench needs the GPU: there is no CPU path to time")
    rt = C.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    nch, blk = a.bench_channels, 1 << 26
    fs, decim, taps, offs, gains = pkg.synth.plan("cfg3_1024ch" if nch > 64 else "cfg2_64ch", nr_channels=nch)
    iq_form = a.form == "iq"
    src = torch.randint(-20000, 20000, (blk, 2), dtype=torch.int16, device="cuda")
    engine_ms = {}
    keep = None
    for want_iq in (False, True):
        eng = pkg.Engine(fs, decim, blk, device=0, flags=b.MFM_F_DEVICE_ONLY | b.MFM_F_TIMING)
        for o, g in zip(offs, gains):
            eng.add_channel(int(o), taps, float(g), want_iq=want_iq)
        eng.commit()
        for _ in range(2 + a.reps):
            dst, cap = eng.acquire_input()
            assert cap >= blk
            assert rt.hipMemcpy(dst, src.data_ptr(), blk * 4, 3) == 0
            torch.cuda.synchronize()
            eng.submit(blk)
            eng.sync()
        engine_ms["iq" if want_iq else "pcm"] = _stats([float(x) for x in eng.launch_ms()[2:]])
        if want_iq == iq_form:
            keep = eng
        else:
            eng.close()
    eng = keep
    d_pcm, stride, nout, d_iq = eng.last_output_device()
    lv = pkg.Level(nch, nout, a.window, form=b.MFM_LEVEL_IQ if iq_form else b.MFM_LEVEL_PCM, device=0)
    pg = pkg.Pocsag(nch, nout, device=0)
    rows, in_stride = (d_iq, 2 * stride) if iq_form else (d_pcm, stride)

    def run_level():
        lv.process_device(rows, in_stride, nout)

    def run_pocsag():
        pg.process_device(d_pcm, stride, nout)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    if a.bench_level_adaptive:   # the line of the adaptive squelch alone, on the same rows
        pg.close()
        bench_level_adaptive(a, pkg, torch, rows, in_stride, nout, timed)
        for o in (lv, eng):
            o.close()
        return
    if a.bench_runrs:   # the two lines of the burst resampler alone, on the same rows
        pg.close()
        bench_runrs(a, pkg, torch, rows, in_stride, nout, timed)
        bench_runrs_dc(a, pkg, torch, rows, in_stride, nout, timed)
        for o in (lv, eng):
            o.close()
        return
    variants = [("level", run_level), ("pocsag_call", run_pocsag)]
    for _, fn in variants:
        timed(fn, 3)
    got = {n: [] for n, _ in variants}
    for rep in range(a.reps):
        order = variants[rep % 2:] + variants[:rep % 2]
        for name, fn in order:
            got[name].append(timed(fn, a.inner))
    lm, lsd = _stats(got["level"])
    pm, psd = _stats(got["pocsag_call"])
    se = math.sqrt(lsd * lsd / a.reps + psd * psd / a.reps)
    in_bytes = nch * nout * (4 if iq_form else 2)
    out_bytes = nch * (nout // a.window) * 40
    res = {"bench": "level_stage", "channels": nch, "form": a.form, "window": a.window, "outputs_per_channel": nout,
           "reps": a.reps, "calls_per_rep": a.inner,
           "level_ms": lm, "level_sd": lsd, "pocsag_call_ms": pm, "pocsag_call_sd": psd,
           "level_minus_pocsag_call_in_se": (lm - pm) / se if se > 0 else None,
           "bytes_read": in_bytes, "bytes_written": out_bytes, "level_fraction_of_hbm_peak": (in_bytes + out_bytes) / (lm * 1e-3) / HBM_PEAK_BPS,
           "engine_launch_ms_pcm_only": engine_ms["pcm"][0], "engine_launch_sd_pcm_only": engine_ms["pcm"][1],
           "engine_launch_ms_with_iq": engine_ms["iq"][0], "engine_launch_sd_with_iq": engine_ms["iq"][1]}
    print(json.dumps(res))
    pg.close()
    bench_level_adaptive(a, pkg, torch, rows, in_stride, nout, timed)
    p0 = None
    for P in [int(x) for x in str(a.gate_preroll).split(",")]:
        line = bench_gate(a, pkg, torch, rt, lv, rows, in_stride, nout, timed, P, p0)
        p0 = line if P == 0 else p0
    if not iq_form:
        bench_runrs(a, pkg, torch, rows, in_stride, nout, timed)
        bench_runrs_dc(a, pkg, torch, rows, in_stride, nout, timed)
        bench_runais(a, pkg, torch)
        bench_runpocsag(a, pkg, torch)
        bench_runbits(a, pkg, torch)
    for o in (lv, eng):
        o.close()


def bench_level_adaptive(a, pkg, torch, rows, in_stride, nout, timed):
    """the level pass with the adaptive squelch off and on (M = the first of --bench-floor-windows, 64; opens at 4, bad below 2
    times the floor) on the rows the level pass was timed on, two objects alternating in one process in rotating order; then the
    adaptive pass at every M of --bench-floor-windows (64, 1 and 1024), alternating likewise.  The two input kernels are the same in all of them: a difference is the finish kernels'"""
    b = pkg.binding
    nch, W, iq_form = a.bench_channels, a.window, a.form == "iq"
    form = b.MFM_LEVEL_IQ if iq_form else b.MFM_LEVEL_PCM

    def make(M):
        lv = pkg.Level(nch, nout, W, form=form, device=0)
        if M:
            lv.set_adaptive(M, 1024, 512, 0)
        return lv

    def ab(variants):
        for _, fn in variants:
            timed(fn, 3)
        got = {n: [] for n, _ in variants}
        for rep in range(a.reps):
            k = rep % len(variants)
            for name, fn in variants[k:] + variants[:k]:
                got[name].append(timed(fn, a.inner))
        return {n: _stats(v) for n, v in got.items()}

    ms = [int(x) for x in str(a.bench_floor_windows).split(",")]
    objs = {M: make(M) for M in [0] + ms}
    run = {M: (lambda lv=lv: lv.process_device(rows, in_stride, nout)) for M, lv in objs.items()}
    first = ab([("fixed", run[0]), ("adaptive", run[ms[0]])])
    (fm, fsd), (am, asd) = first["fixed"], first["adaptive"]
    se = math.sqrt(fsd * fsd / a.reps + asd * asd / a.reps)
    d = am - fm
    by_m = ab([(str(M), run[M]) for M in ms])
    out = {"bench": "level_adaptive_stage", "channels": nch, "form": a.form, "window": W, "outputs_per_channel": nout,
           "windows_per_call": nout // W, "reps": a.reps, "calls_per_rep": a.inner, "floor_windows": ms[0], "open_q8": 1024, "close_q8": 512,
           "fixed_ms": fm, "fixed_sd": fsd, "adaptive_ms": am, "adaptive_sd": asd, "adaptive_over_fixed": am / fm,
           "difference_ms": d, "difference_se": se,
           "verdict": "neutral" if abs(d) <= 2.0 * se else ("faster" if d < 0 else "slower"),
           "adaptive_ms_by_floor_windows": {str(M): {"ms": by_m[str(M)][0], "sd": by_m[str(M)][1]} for M in ms}}
    print(json.dumps(out))
    for lv in objs.values():
        lv.close()


def bench_gate(a, pkg, torch, rt, lv, rows, in_stride, nout, timed, P=0, p0=None):
    """the gate on whole windows of the rows the level pass was timed on: nb = (nout // W) * W samples per call, so that every
    call completes the same windows and the carry stays empty.  Its records are those of one level call on these nb samples;
    later calls find their .window behind the gate's position, which raises the out-of-step flag and changes no work.
    With P pre-roll windows every call emits the last P windows of the call before it (the same rows and records) and all but the
    last P of its own, by the dilated mask; p0 is the P = 0 line of the same run."""
    b = pkg.binding
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    nch, W, iq_form = a.bench_channels, a.window, a.form == "iq"
    E = 2 if iq_form else 1
    nw = nout // W
    nb = nw * W
    form = b.MFM_LEVEL_IQ if iq_form else b.MFM_LEVEL_PCM
    probe = pkg.Level(nch, nout, W, form=form, device=0)
    probe.process_device(rows, in_stride, nb)
    energy = probe.fetch()["energy"]
    probe.close()
    thr = int(np.median(energy))
    sq = pkg.Level(nch, nout, W, form=form, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
    sq.process_device(rows, in_stride, nb)
    scene = sq.fetch()
    d_scene, scene_stride, scene_nw, _ = sq.device_view()
    assert scene_nw == nw
    masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
    keep, recs = [], {}
    for name in ("all_closed", "all_open"):
        r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
        r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
        r["open"] = masks[name]
        t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
        keep.append(t)
        recs[name] = (t.data_ptr(), nw)
    recs["scene"] = (d_scene, scene_stride)
    gate = pkg.Gate(nch, nout, W, elems_per_sample=E, device=0, preroll_windows=P)
    sink = torch.empty(nch * nb * E, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()

    def run_level():
        lv.process_device(rows, in_stride, nb)

    out = {"bench": "gate_stage", "channels": nch, "form": a.form, "window": W, "samples_per_channel": nb, "windows_per_channel": nw,
           "reps": a.reps, "calls_per_rep": a.inner, "row_base_mod_16": int(rows % 16), "in_stride_elems_mod_8": int(in_stride % 8),
           "window_elems_mod_8": int(W * E % 8), "preroll": P,
           "history_bytes": 2 * nch * (((P + 1) * W * E + 7) & ~7) * 2}
    # which alignment path the copy takes: the payload slot of a window is a multiple of W * E elements off a 16-byte base, its
    # source (window k of a row) lies at row base + k * W * E elements
    aligned = rows % 16 == 0 and in_stride % 8 == 0 and (W * E) % 8 == 0
    out["copy_path"] = "16-byte stores fed by aligned 16-byte loads" if aligned else "16-byte stores fed by unaligned 16-byte loads"
    for name in ("all_closed", "all_open", "scene"):
        d_rec, rstride = recs[name]
        m = masks[name].astype(bool)
        if P:  # the steady state: the records in front of a call are the last P of the same mask
            ext = np.concatenate([m[:, nw - P:], m], axis=1)
            m = np.logical_or.reduce([ext[:, t:t + nw] for t in range(P + 1)])
        nbytes = int(m.sum()) * W * E * 2

        def run_gate():
            gate.process_device(rows, in_stride, nb, d_rec, rstride, nw)

        def run_copy():
            if nbytes:
                assert rt.hipMemcpyAsync(sink.data_ptr(), rows, nbytes, 3, None) == 0

        variants = [("gate", run_gate), ("copy", run_copy), ("level", run_level)]
        for _, fn in variants:
            timed(fn, 3)
        got = {n: [] for n, _ in variants}
        for rep in range(a.reps):
            k = rep % len(variants)
            for vname, fn in variants[k:] + variants[:k]:
                got[vname].append(timed(fn, a.inner))
        (gm, gsd), (cm, csd), (lm, lsd) = _stats(got["gate"]), _stats(got["copy"]), _stats(got["level"])
        out[name] = {"open_windows": nbytes // (W * E * 2), "payload_bytes": nbytes, "gate_ms": gm, "gate_sd": gsd,
                     "d2d_copy_ms": cm if nbytes else None, "d2d_copy_sd": csd if nbytes else None,
                     "gate_over_copy": gm / cm if nbytes else None, "level_ms": lm, "level_sd": lsd,
                     "gate_payload_gbps": nbytes / (gm * 1e-3) / 1e9}
        if P and p0:
            out[name]["gate_ms_over_p0"] = gm / p0[name]["gate_ms"]
    print(json.dumps(out))
    for o in (gate, sq):
        o.close()
    return out


def _runrs_bench_scene(a, pkg, torch, rows, in_stride, nout):
    """what bench_runrs and bench_runrs_dc time on: 4/5 with 81 taps on whole windows of the PCM rows, and the level records of the
    three masks (all closed, all open, a squelch at the median window energy) on the device"""
    b = pkg.binding
    nch, W = a.bench_channels, a.window
    nw = nout // W
    nb = nw * W
    taps = (np.hanning(81) * 0.2 * 16384.0).astype(np.int16)
    probe = pkg.Level(nch, nout, W, device=0)
    probe.process_device(rows, in_stride, nb)
    energy = probe.fetch()["energy"]
    probe.close()
    thr = int(np.median(energy))
    sq = pkg.Level(nch, nout, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
    sq.process_device(rows, in_stride, nb)
    scene = sq.fetch()
    d_scene, scene_stride, _, _ = sq.device_view()
    masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
    keep, recs = [], {"scene": (d_scene, scene_stride)}
    for name in ("all_closed", "all_open"):
        r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
        r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
        r["open"] = masks[name]
        t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
        keep.append(t)
        recs[name] = (t.data_ptr(), nw)
    return taps, nw, nb, masks, recs, (sq, keep)


def _runrs_totals(pkg, rr):
    """(runs, output samples) of the last call, from the totals alone: the payload stays on the device"""
    try:
        rr.fetch(max_runs=0, max_elems=0)
        return 0, 0
    except pkg.MfmError as err:
        if err.code != pkg.binding.MFM_E_NOMEM:
            raise
        return err.needed


def bench_runrs(a, pkg, torch, rows, in_stride, nout, timed):
    """the burst resampler behind the gate, 4/5 with 81 taps, on whole windows of the PCM rows.  Per mask one gate call leaves its
    runs and payload in place and the stage is timed on that device view over and over: from the second call on a run's
    first_window is behind what its channel expects, so every call begins every stretch anew and does the same work.  The plain
    resampler (v_dot2 form forced) on the full rows alternates with it in the same process, in rotating order."""
    nch, W, I, D = a.bench_channels, a.window, 4, 5
    taps, nw, nb, masks, recs, (sq, _keep) = _runrs_bench_scene(a, pkg, torch, rows, in_stride, nout)
    plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True)
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=nout, device=0)

    def run_plain():
        plain.process_device(rows, in_stride, nb)

    out = {"bench": "runrs_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner}
    for name in ("all_closed", "all_open", "scene"):
        gate = pkg.Gate(nch, nout, W, device=0)
        gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
        view = gate.device_view()

        def run_rr():
            rr.process_device(*view)

        variants = [("runrs", run_rr), ("plain", run_plain)]
        for _, fn in variants:
            timed(fn, 3)
        nr_runs, nr_out = _runrs_totals(pkg, rr)
        got = {n: [] for n, _ in variants}
        for rep in range(a.reps):
            k = rep % len(variants)
            for vname, fn in variants[k:] + variants[:k]:
                got[vname].append(timed(fn, a.inner))
        (rm, rsd), (pm, psd) = _stats(got["runrs"]), _stats(got["plain"])
        ratio = rm / pm
        ratio_se = ratio * math.sqrt(rsd * rsd / a.reps / (rm * rm) + psd * psd / a.reps / (pm * pm))
        out[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(nr_runs),
                     "input_samples": int(masks[name].astype(bool).sum()) * W, "output_samples": int(nr_out), "runrs_ms": rm, "runrs_sd": rsd, "plain_dot2_ms": pm, "plain_dot2_sd": psd,
                     "runrs_over_plain": ratio, "runrs_over_plain_se": ratio_se}
        gate.close()
    print(json.dumps(out))
    for o in (rr, plain, sq):
        o.close()


def bench_runrs_dc(a, pkg, torch, rows, in_stride, nout, timed):
    """the burst resampler's DC blocker on the scene of bench_runrs: per mask the burst resampler with the blocker (pole 0.999), the
    burst resampler without it and the plain resampler (v_dot2 form forced) with dc_block on the full rows, alternating in one
    process in rotating order.  As there, every timed call begins every stretch anew, so each does the same work"""
    nch, W, I, D, pole = a.bench_channels, a.window, 4, 5, 0.999
    taps, nw, nb, masks, recs, (sq, _keep) = _runrs_bench_scene(a, pkg, torch, rows, in_stride, nout)
    plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True, dc_pole=pole)
    rr_dc = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=nout, device=0)
    rr_dc.set_dc_block(pole)
    rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=nout, device=0)

    def run_plain():
        plain.process_device(rows, in_stride, nb)

    out = {"bench": "runrs_dc_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "pole": pole, "dc_p": rr_dc.dc_block()[1], "reps": a.reps, "calls_per_rep": a.inner}
    for name in ("all_closed", "all_open", "scene"):
        gate = pkg.Gate(nch, nout, W, device=0)
        gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
        view = gate.device_view()

        def run_dc():
            rr_dc.process_device(*view)

        def run_rr():
            rr.process_device(*view)

        variants = [("runrs_dc", run_dc), ("runrs", run_rr), ("plain_dc", run_plain)]
        for _, fn in variants:
            timed(fn, 3)
        nr_runs, nr_out = _runrs_totals(pkg, rr_dc)
        got = {n: [] for n, _ in variants}
        for rep in range(a.reps):
            k = rep % len(variants)
            for vname, fn in variants[k:] + variants[:k]:
                got[vname].append(timed(fn, a.inner))
        (dm, dsd), (rm, rsd), (pm, psd) = _stats(got["runrs_dc"]), _stats(got["runrs"]), _stats(got["plain_dc"])
        cost_se = math.sqrt(dsd * dsd / a.reps + rsd * rsd / a.reps)
        ratio = dm / pm
        ratio_se = ratio * math.sqrt(dsd * dsd / a.reps / (dm * dm) + psd * psd / a.reps / (pm * pm))
        out[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(nr_runs), "output_samples": int(nr_out),
                     "runrs_dc_ms": dm, "runrs_dc_sd": dsd, "runrs_ms": rm, "runrs_sd": rsd, "plain_dot2_dc_ms": pm, "plain_dot2_dc_sd": psd,
                     "dc_cost_ms": dm - rm, "dc_cost_se": cost_se, "runrs_dc_over_plain_dc": ratio, "runrs_dc_over_plain_dc_se": ratio_se}
        gate.close()
    print(json.dumps(out))
    for o in (rr_dc, rr, plain, sq):
        o.close()


def _busy_rows(pkg, nch, n):
    """[nch][n] int16 at 60 kHz: AIS frames of three types, CRC rejects and stretches without transitions on every channel (eight
    different streams, rotated from channel to channel)"""
    sy = pkg.synth
    rng = np.random.RandomState(5)
    pl = [sy.ais_type1(mmsi=123456789, sog=123), sy.ais_type4(mmsi=111222333), sy.ais_type5(mmsi=987654321, ship_name="BENCH")]
    n48 = n * 4 // 5 + 8
    base = []
    for k in range(8):
        frames = []
        while sum(len(f) for f in frames) * 5 < n48:
            j = int(rng.randint(0, 5))
            if j < 3:
                frames.append(sy.ais_frame_bits(pl[j]))
            elif j == 3:
                frames.append(sy.ais_frame_bits(pl[int(rng.randint(0, 3))], fcs=int(rng.randint(0, 65536))))
            else:
                frames.append(np.ones(int(rng.randint(1, 400)), np.uint8))
        x = sy.ais_pcm(sy.ais_bits(frames, gap_bits=2), noise=400.0, phase=k % 5, seed=k)
        base.append(np.repeat(x, 5)[::4][:n])
    return np.stack([np.roll(base[c % 8], 977 * (c // 8)) for c in range(nch)])


def bench_runais(a, pkg, torch):
    """burst resampler -> burst AIS stage on the device view one gate call left (every call begins every stretch anew, as in
    bench_runrs, so every call does the same work) against mfm_resampler (v_dot2 form) -> mfm_ais on the full rows; the two chains
    alternate in one process in rotating order"""
    b = pkg.binding
    nch, W, I, D = a.bench_channels, a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runais_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner, "search": "M words computed in the walker"}
    rng = np.random.RandomState(1)
    for rows_name in ("idle", "busy"):
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16) if rows_name == "idle" else _busy_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
        keep, recs = [], {"scene": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True)
        ais = pkg.Ais(nch, plain.max_out(), device=0)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        ra = pkg.RunAis.behind(rr)

        def run_plain():
            yptr, ystride, ny = plain.process_device(rows, in_stride, nb)
            ais.process_device(yptr, ystride, ny)

        res = {}
        for name in ("all_closed", "scene", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_burst():
                rr.process_device(*view)
                ra.process_device(*rr.device_view())

            variants = [("burst", run_burst), ("plain", run_plain)]
            for _, fn in variants:
                timed(fn, 3)
            nr_events, plain_events = len(ra.fetch()), len(ais.fetch_events())
            got = {v: [] for v, _ in variants}
            for rep in range(a.reps):
                k = rep % len(variants)
                for vname, fn in variants[k:] + variants[:k]:
                    got[vname].append(timed(fn, a.inner))
            (bm, bsd), (pm, psd) = _stats(got["burst"]), _stats(got["plain"])
            ratio = bm / pm
            ratio_se = ratio * math.sqrt(bsd * bsd / a.reps / (bm * bm) + psd * psd / a.reps / (pm * pm))
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "burst_events_per_call": nr_events,
                         "plain_events_last_call": plain_events, "burst_ms": bm, "burst_sd": bsd, "plain_ms": pm, "plain_sd": psd,
                         "burst_over_plain": ratio, "burst_over_plain_se": ratio_se}
            gate.close()
        out[rows_name] = res
        for o in (ra, rr, ais, plain, sq):
            o.close()
        del d_rows, keep
    print(json.dumps(out))


def _busy_pocsag_rows(pkg, nch, n):
    """[nch][n] int16 at 48 kHz (38 400 Hz behind the 4/5 resampler): POCSAG transmissions at 512, 1200 and 2400 baud back to
    back with short noise gaps on every channel (six different streams, rotated from channel to channel)"""
    sy = pkg.synth
    rng = np.random.RandomState(6)
    msgs = [(0x12345, 3, 2, sy.pocsag_alpha_words("HELLO MI355X\x04")), (0x00777, 5, 0, sy.pocsag_numeric_words("0123-456 [9]")),
            (0x3FFFF, 0, 3, sy.pocsag_alpha_words("The quick brown fox jumps over the lazy dog 0123456789\x03"))]
    n38 = n * 4 // 5 + 8
    base = []
    for k in range(6):
        parts, have = [], 0
        while have < n38:
            baud = (2400, 1200, 2400, 512, 2400, 1200)[(k + len(parts)) % 6]
            pick = [msgs[int(j)] for j in rng.randint(0, 3, 1 + int(rng.randint(0, 3)))]
            parts.append(sy.pocsag_pcm(sy.pocsag_bits(sy.pocsag_batches(pick)), baud, noise=600.0, lead=int(rng.randint(200, 3000)),
                                       trail=2600, seed=10 * k + len(parts)))
            have += parts[-1].size
        base.append(np.repeat(np.concatenate(parts)[:n38], 5)[::4][:n])
    return np.stack([np.roll(base[c % 6], 1013 * (c // 6)) for c in range(nch)])


def bench_runpocsag(a, pkg, torch):
    """burst resampler -> burst POCSAG stage on the device view one gate call left (every call begins every stretch anew, as in
    bench_runrs, so every call does the same work) against mfm_resampler (v_dot2 form) -> mfm_pocsag on the full rows; the two
    chains alternate in one process in rotating order.  The events of a call's first runs are compared with the host twin's"""
    b = pkg.binding
    nch, W, I, D = a.bench_channels, a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runpocsag_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner,
           "search": "match planes and summary (rp_match_kernel), EXACT words in the walker"}
    rng = np.random.RandomState(1)
    sample_ok, sample_events = True, 0
    for rows_name in ("idle", "busy"):
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16) if rows_name == "idle" else _busy_pocsag_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
        keep, recs = [], {"scene": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True)
        pg = pkg.Pocsag(nch, plain.max_out(), device=0)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rp = pkg.RunPocsag.behind(rr)

        def run_plain():
            yptr, ystride, ny = plain.process_device(rows, in_stride, nb)
            pg.process_device(yptr, ystride, ny)

        res = {}
        for name in ("all_closed", "scene", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_burst():
                rr.process_device(*view)
                rp.process_device(*rr.device_view())

            variants = [("burst", run_burst), ("plain", run_plain)]
            for _, fn in variants:
                timed(fn, 3)
            ev = rp.fetch()
            plain_events = len(pg.fetch_events())
            # a sample against the twin: the call's first runs (each begins its stretch, so each stands alone)
            runs, payload = rr.fetch()
            k = 0
            while k < min(len(runs), 6) and int(runs["out_offset"][k]) + int(runs["nr_out"][k]) <= 1 << 20:
                k += 1
            if k:
                assert (runs["flags"][:k] & 1).all()
                want = b.hosttwin_runpocsag_call(b.hosttwin_runpocsag_state(nch), runs[:k], payload[:int(runs["out_offset"][k - 1]) + int(runs["nr_out"][k - 1])])
                got = ev[ev["run"] < k]
                sample_ok = sample_ok and got.tobytes() == want.tobytes()
                sample_events += len(want)
            got_t = {v: [] for v, _ in variants}
            for rep in range(a.reps):
                j = rep % len(variants)
                for vname, fn in variants[j:] + variants[:j]:
                    got_t[vname].append(timed(fn, a.inner))
            (bm, bsd), (pm, psd) = _stats(got_t["burst"]), _stats(got_t["plain"])
            ratio = bm / pm
            ratio_se = ratio * math.sqrt(bsd * bsd / a.reps / (bm * bm) + psd * psd / a.reps / (pm * pm))
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(len(runs)), "burst_events_per_call": int(len(ev)),
                         "plain_events_last_call": plain_events, "burst_ms": bm, "burst_sd": bsd, "plain_ms": pm, "plain_sd": psd,
                         "burst_over_plain": ratio, "burst_over_plain_se": ratio_se}
            gate.close()
        out[rows_name] = res
        for o in (rp, rr, pg, plain, sq):
            o.close()
        del d_rows, keep
    out["sample_equals_twin"] = bool(sample_ok)
    out["sample_events"] = int(sample_events)
    print(json.dumps(out))


def _busy_flex_rows(pkg, nch, n):
    """[nch][n] int16 at 25 kHz (16 000 Hz behind the 16/25 resampler): FLEX frames of the four codings back to back on every
    channel (four different streams, rotated from channel to channel)"""
    sy = pkg.synth
    recs = [dict(kind="alnum", capcode=1000 + i, text="THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG %d" % i) for i in range(4)]
    frames = []
    for k in range(4):
        ph = {p: sy.flex_phase_words(recs) for p in sy.FLEX_CODINGS[k]["phases"]}
        frames.append(sy.flex_pcm([sy.flex_frame_levels(k, 1, k, ph)], noise=300, seed=k, rate=25000))
    base = [np.concatenate([frames[(k + i) % 4] for i in range(n // frames[0].size + 2)])[:n] for k in range(4)]
    return np.stack([np.roll(base[c % 4], 1013 * (c // 4)) for c in range(nch)])


def bench_runflex(a, pkg, torch):
    """burst resampler -> burst FLEX stage on the device view one gate call left (every call begins every stretch anew, as in
    bench_runrs, so every call does the same work) against mfm_resampler (v_dot2 form) -> mfm_flex on the full rows; the two
    chains alternate in one process in rotating order.  The events and words of a call's first runs are compared with the host
    twin's"""
    b = pkg.binding
    nch, W, I, D = a.bench_channels, a.window, 16, 25
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16 * 16384.0).astype(np.int16)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runflex_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner,
           "search": "match plane and summary (rf_match_kernel)"}
    rng = np.random.RandomState(1)
    sample_ok, sample_events = True, 0
    for rows_name in ("idle", "busy"):
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16) if rows_name == "idle" else _busy_flex_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "half_open": scene["open"]}
        keep, recs = [], {"half_open": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True)
        fx = pkg.Flex(nch, plain.max_out(), device=0)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rf = pkg.RunFlex.behind(rr)

        def run_plain():
            yptr, ystride, ny = plain.process_device(rows, in_stride, nb)
            fx.process_device(yptr, ystride, ny)

        res = {}
        for name in ("all_closed", "half_open", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_burst():
                rr.process_device(*view)
                rf.process_device(*rr.device_view())

            variants = [("burst", run_burst), ("plain", run_plain)]
            for _, fn in variants:
                timed(fn, 3)
            ev, fw = rf.fetch()
            plain_events = len(fx.fetch_events()[0])
            # a sample against the twin: the call's first runs (each begins its stretch, so each stands alone)
            runs, payload = rr.fetch()
            k = 0
            while k < min(len(runs), 6) and int(runs["out_offset"][k]) + int(runs["nr_out"][k]) <= 1 << 20:
                k += 1
            if k:
                assert (runs["flags"][:k] & 1).all()
                want = b.hosttwin_runflex_call(b.hosttwin_runflex_state(nch), runs[:k], payload[:int(runs["out_offset"][k - 1]) + int(runs["nr_out"][k - 1])])
                got = ev[ev["run"] < k]
                sample_ok = sample_ok and got.tobytes() == want[0].tobytes() and fw[:len(want[1])].tobytes() == want[1].tobytes()
                sample_events += len(want[0])
            got_t = {v: [] for v, _ in variants}
            for rep in range(a.reps):
                j = rep % len(variants)
                for vname, fn in variants[j:] + variants[:j]:
                    got_t[vname].append(timed(fn, a.inner))
            (bm, bsd), (pm, psd) = _stats(got_t["burst"]), _stats(got_t["plain"])
            ratio = bm / pm
            ratio_se = ratio * math.sqrt(bsd * bsd / a.reps / (bm * bm) + psd * psd / a.reps / (pm * pm))
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(len(runs)), "burst_events_per_call": int(len(ev)),
                         "burst_frames_per_call": int(len(fw)), "plain_events_last_call": plain_events, "burst_ms": bm, "burst_sd": bsd,
                         "plain_ms": pm, "plain_sd": psd, "burst_over_plain": ratio, "burst_over_plain_se": ratio_se}
            gate.close()
        out[rows_name] = res
        for o in (rf, rr, fx, plain, sq):
            o.close()
        del d_rows, keep
    out["sample_equals_twin"] = bool(sample_ok)
    out["sample_events"] = int(sample_events)
    print(json.dumps(out))


def bench_runroute(a, pkg, torch):
    """the run router on the device view one gate call left, at 64 and 1024 channels, idle (noise) rows, the three masks of
    runrs_stage.  (a) the router call alone beside the burst resampler's call on an all-closed view (a launch-overhead yardstick),
    (b) a two-protocol capture, the first half of the channels POCSAG (4/5) and the second half FLEX (16/25): router + one burst
    chain per route against two whole chains that each read every channel's runs.  Everything alternates in one process in
    rotating order; every call begins every stretch anew, as in bench_runrs, so every call does the same work"""
    b = pkg.binding
    W, n = a.window, 1 << 15
    nw = n // W
    nb = nw * W
    ptaps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)
    ftaps = np.round(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16 * 16384.0).astype(np.int16)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    def ab(variants):
        for _, fn in variants:
            timed(fn, 3)
        got = {v: [] for v, _ in variants}
        for rep in range(a.reps):
            j = rep % len(variants)
            for vname, fn in variants[j:] + variants[:j]:
                got[vname].append(timed(fn, a.inner))
        return {v: _stats(x) for v, x in got.items()}

    def verdict(x, y):
        """x against y: the difference, its standard error, and tools/exp/ab.py's rule"""
        d, se = x[0] - y[0], math.sqrt(x[1] * x[1] / a.reps + y[1] * y[1] / a.reps)
        return {"difference_ms": d, "difference_se": se, "verdict": "neutral" if abs(d) <= 2.0 * se else ("faster" if d < 0 else "slower")}

    out = {"bench": "runroute_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "reps": a.reps,
           "calls_per_rep": a.inner, "routes": {"0": "pocsag 4/5, 41 taps, the first half of the channels",
                                                "1": "flex 16/25, 101 taps, the second half"}}
    rng = np.random.RandomState(1)
    for nch in (64, 1024):
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16)
        d_rows = torch.from_numpy(host).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "half_open": scene["open"]}
        keep, recs = [], {"half_open": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        table = np.where(np.arange(nch) < nch // 2, 0, 1).astype(np.uint8)
        router = pkg.RunRouter.behind(table, 2, n, W)
        chains = {}
        for side in ("routed", "full"):
            rp_rr = pkg.RunResampler(nch, ptaps, 4, 5, W, max_in_samples=n, device=0)
            rf_rr = pkg.RunResampler(nch, ftaps, 16, 25, W, max_in_samples=n, device=0)
            chains[side] = (rp_rr, pkg.RunPocsag.behind(rp_rr), rf_rr, pkg.RunFlex.behind(rf_rr))
        closed = pkg.Gate(nch, n, W, device=0)
        closed.process_device(rows, in_stride, nb, recs["all_closed"][0], recs["all_closed"][1], nw)
        closed_view = closed.device_view()
        rr_closed = pkg.RunResampler(nch, ptaps, 4, 5, W, max_in_samples=n, device=0)
        res = {}
        for name in ("all_closed", "half_open", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_router():
                router.process_device(*view)

            def run_rr_closed():
                rr_closed.process_device(*closed_view)

            def run_chains(side, views):
                rp_rr, rp, rf_rr, rf = chains[side]
                rp_rr.process_device(*views[0])
                rp.process_device(*rp_rr.device_view())
                rf_rr.process_device(*views[1])
                rf.process_device(*rf_rr.device_view())

            def run_routed():
                router.process_device(*view)
                run_chains("routed", (router.device_view(0), router.device_view(1)))

            def run_full():
                run_chains("full", (view, view))

            alone = ab([("router", run_router), ("runrs_all_closed", run_rr_closed)])
            both = ab([("routed", run_routed), ("full", run_full)])
            runs = [len(router.fetch(k)[0]) for k in range(2)]
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "gate_runs": sum(runs),
                         "route_runs": runs, "router_ms": alone["router"][0], "router_sd": alone["router"][1],
                         "runrs_all_closed_ms": alone["runrs_all_closed"][0], "runrs_all_closed_sd": alone["runrs_all_closed"][1],
                         "routed_ms": both["routed"][0], "routed_sd": both["routed"][1], "full_ms": both["full"][0], "full_sd": both["full"][1],
                         "routed_over_full": both["routed"][0] / both["full"][0], "routed_against_full": verdict(both["routed"], both["full"])}
            gate.close()
        out[str(nch)] = res
        for side in chains.values():
            for o in (side[1], side[3], side[0], side[2]):
                o.close()
        for o in (rr_closed, closed, router, sq):
            o.close()
        del d_rows, keep
    print(json.dumps(out))


def bench_runroute_pack(a, pkg, torch):
    """packed routes against zero-copy routes (RunRouter(sets=..., pack=True / False)) on the scene of bench_runroute: 64 and 1024
    channels in 2 routes (POCSAG 4/5 and FLEX 16/25 halves) and 1024 channels in 8 routes (eighths, POCSAG and FLEX in turn), the
    three masks.  Per shape and mask, alternating in one process in rotating order: (a) router + one chain per route, the chains
    sized by route_caps() of either form; (b) the two router calls alone, whose difference is the pack copy and the partition's
    window sums together - an upper bound of the copy kernel's time, beside the bytes it reads and writes.  The device bytes of
    either form are the drop of free device memory across the creation of its objects"""
    b = pkg.binding
    W, n = a.window, 1 << 15
    nw = n // W
    nb = nw * W
    taps = {"pocsag": (np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16), 4, 5),
            "flex": (np.round(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16 * 16384.0).astype(np.int16), 16, 25)}

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    def ab(variants):
        for _, fn in variants:
            timed(fn, 3)
        got = {v: [] for v, _ in variants}
        for rep in range(a.reps):
            j = rep % len(variants)
            for vname, fn in variants[j:] + variants[:j]:
                got[vname].append(timed(fn, a.inner))
        return {v: (_stats(x)[0], _stats(x)[1] / math.sqrt(a.reps)) for v, x in got.items()}   # mean, standard error

    def verdict(x, y):
        """x against y: the difference, its standard error, and tools/exp/ab.py's rule"""
        d, se = x[0] - y[0], math.sqrt(x[1] * x[1] + y[1] * y[1])
        return {"difference_ms": d, "difference_se": se, "verdict": "neutral" if abs(d) <= 2.0 * se else ("faster" if d < 0 else "slower")}

    def allocated(make):
        """(the object, the device bytes its creation took)"""
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        o = make()
        torch.cuda.synchronize()
        return o, free0 - torch.cuda.mem_get_info()[0]

    out = {"bench": "runroute_pack_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "reps": a.reps,
           "calls_per_rep": a.inner, "routes": "route k: channels [k C / K, (k + 1) C / K); pocsag 4/5, 41 taps for even k, flex 16/25, 101 taps for odd k",
           "times": "mean and standard error of the mean over reps, ms per call",
           "copy_bytes": "read and written by rt_pack_kernel: 2 * 2 bytes * the routes' payload elements"}
    only = a.pack_only.split("/") if a.pack_only else None   # one case, for a kernel trace of its own
    rng = np.random.RandomState(1)
    for nch, K in ((64, 2), (1024, 2), (1024, 8)):
        if only and only[0] != "%dx%d" % (nch, K):
            continue
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16)
        d_rows = torch.from_numpy(host).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "half_open": scene["open"]}
        keep, recs = [], {"half_open": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        sets = (1 << (np.arange(nch) * K // nch)).astype(np.uint8)
        stages = ["pocsag" if k % 2 == 0 else "flex" for k in range(K)]
        forms, device_bytes = {}, {}
        for form in ("zero_copy", "packed"):
            router, total = allocated(lambda: pkg.RunRouter.behind(None, K, n, W, sets=sets, pack=form == "packed"))
            chains = []
            for k in range(K):
                co, I, D = taps[stages[k]]
                nc, mw, mr = router.route_caps(k)
                rr, got = allocated(lambda: pkg.RunResampler(nc, co, I, D, W, max_in_samples=n, max_windows=mw, max_runs=mr, device=0))
                total += got
                st, got = allocated(lambda: (pkg.RunPocsag if stages[k] == "pocsag" else pkg.RunFlex).behind(rr))
                total += got
                chains.append((rr, st))
            forms[form], device_bytes[form] = (router, chains), int(total)
        res = {"device_bytes": device_bytes, "route_caps": {f: [list(forms[f][0].route_caps(k)) for k in range(K)] for f in forms}}
        for name in ("all_closed", "half_open", "all_open"):
            if only and only[1] != name:
                continue
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_router(form):
                forms[form][0].process_device(*view)

            def run_form(form):
                router, chains = forms[form]
                router.process_device(*view)
                for k, (rr, st) in enumerate(chains):
                    rr.process_device(*router.device_view(k))
                    st.process_device(*rr.device_view())

            both = ab([("packed", lambda: run_form("packed")), ("zero_copy", lambda: run_form("zero_copy"))])
            alone = ab([("packed", lambda: run_router("packed")), ("zero_copy", lambda: run_router("zero_copy"))])
            run_form("packed")
            run_form("zero_copy")
            elems = [forms["packed"][0].fetch(k)[1] for k in range(K)]
            runs = [len(forms["packed"][0].fetch(k)[0]) for k in range(K)]
            same = all(forms["packed"][1][k][0].fetch()[1].tobytes() == forms["zero_copy"][1][k][0].fetch()[1].tobytes() for k in (0, K - 1))
            copy_ms, copy_se = alone["packed"][0] - alone["zero_copy"][0], math.sqrt(alone["packed"][1] ** 2 + alone["zero_copy"][1] ** 2)
            copy_bytes = 4 * sum(elems)
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "route_runs": runs, "route_elems": elems,
                         "packed_ms": both["packed"][0], "packed_se": both["packed"][1], "zero_copy_ms": both["zero_copy"][0],
                         "zero_copy_se": both["zero_copy"][1], "packed_over_zero_copy": both["packed"][0] / both["zero_copy"][0],
                         "packed_against_zero_copy": verdict(both["packed"], both["zero_copy"]),
                         "router_packed_ms": alone["packed"][0], "router_packed_se": alone["packed"][1],
                         "router_zero_copy_ms": alone["zero_copy"][0], "router_zero_copy_se": alone["zero_copy"][1],
                         "copy_ms_upper_bound": copy_ms, "copy_se": copy_se, "copy_bytes": copy_bytes,
                         "copy_gb_per_s_lower_bound": (copy_bytes / (copy_ms * 1e-3) / 1e9) if copy_bytes and copy_ms > 0 else None,
                         "resampled_payloads_equal": bool(same)}
            gate.close()
        out["%dx%d" % (nch, K)] = res
        for router, chains in forms.values():
            for rr, st in chains:
                st.close()
                rr.close()
            router.close()
        sq.close()
        del d_rows, keep
    print(json.dumps(out))


def bench_runroute_local(a, pkg, torch):
    """the three forms of the run router on the cases of bench_runroute_pack (64 and 1024 channels in 2 routes, 1024 in 8; all
    closed, half open, all open): zero-copy with global channel numbers (RunRouter(sets=...)), packed (pack=True) and local
    (local=True, the chains through the view entries).  Per shape and mask, alternating in one process in rotating order: (a)
    router + one chain per route, the chains sized by route_caps() of each form; (b) the three router calls alone.  The device
    bytes of a form are the drop of free device memory across the creation of its objects"""
    b = pkg.binding
    W, n = a.window, 1 << 15
    nw = n // W
    nb = nw * W
    taps = {"pocsag": (np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16), 4, 5),
            "flex": (np.round(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16 * 16384.0).astype(np.int16), 16, 25)}
    names = ("zero_copy", "packed", "local")

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    def ab(variants):
        for _, fn in variants:
            timed(fn, 3)
        got = {v: [] for v, _ in variants}
        for rep in range(a.reps):
            j = rep % len(variants)
            for vname, fn in variants[j:] + variants[:j]:
                got[vname].append(timed(fn, a.inner))
        return {v: (_stats(x)[0], _stats(x)[1], _stats(x)[1] / math.sqrt(a.reps)) for v, x in got.items()}   # mean, sd, standard error

    def verdict(x, y):
        """x against y: the difference, its standard error, and tools/exp/ab.py's rule"""
        d, se = x[0] - y[0], math.sqrt(x[2] * x[2] + y[2] * y[2])
        return {"difference_ms": d, "difference_se": se, "ratio": x[0] / y[0],
                "verdict": "neutral" if abs(d) <= 2.0 * se else ("faster" if d < 0 else "slower")}

    def allocated(make):
        """(the object, the device bytes its creation took)"""
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        o = make()
        torch.cuda.synchronize()
        return o, free0 - torch.cuda.mem_get_info()[0]

    out = {"bench": "runroute_local_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "reps": a.reps,
           "calls_per_rep": a.inner, "routes": "route k: channels [k C / K, (k + 1) C / K); pocsag 4/5, 41 taps for even k, flex 16/25, 101 taps for odd k",
           "times": "[mean, standard deviation, standard error of the mean] over reps, ms per call",
           "forms": "zero_copy: global channel numbers, chains of all channels; packed: MFM_RUNROUTE_F_PACK; local: mfm_runroute_create_local + view entries"}
    rng = np.random.RandomState(1)
    for nch, K in ((64, 2), (1024, 2), (1024, 8)):
        host = rng.randint(-3000, 3001, size=(nch, n)).astype(np.int16)
        d_rows = torch.from_numpy(host).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "half_open": scene["open"]}
        keep, recs = [], {"half_open": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        sets = (1 << (np.arange(nch) * K // nch)).astype(np.uint8)
        stages = ["pocsag" if k % 2 == 0 else "flex" for k in range(K)]
        forms, device_bytes = {}, {}
        for form in names:
            router, total = allocated(lambda: pkg.RunRouter.behind(None, K, n, W, sets=sets, pack=form == "packed", local=form == "local"))
            chains = []
            for k in range(K):
                co, I, D = taps[stages[k]]
                nc, mw, mr = router.route_caps(k)
                rr, got = allocated(lambda: pkg.RunResampler(nc, co, I, D, W, max_in_samples=n, max_windows=mw, max_runs=mr, device=0))
                total += got
                st, got = allocated(lambda: (pkg.RunPocsag if stages[k] == "pocsag" else pkg.RunFlex).behind(rr))
                total += got
                chains.append((rr, st))
            forms[form], device_bytes[form] = (router, chains), int(total)
        res = {"device_bytes": device_bytes, "route_caps": {f: [list(forms[f][0].route_caps(k)) for k in range(K)] for f in forms}}
        for name in ("all_closed", "half_open", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_router(form):
                forms[form][0].process_device(*view)

            def run_form(form):
                router, chains = forms[form]
                router.process_device(*view)
                for k, (rr, st) in enumerate(chains):
                    if form == "local":
                        rr.process_view_device(*router.device_view(k), router.bound_view())
                    else:
                        rr.process_device(*router.device_view(k))
                    st.process_device(*rr.device_view())

            both = ab([(f, lambda f=f: run_form(f)) for f in names])
            alone = ab([(f, lambda f=f: run_router(f)) for f in names])
            for f in names:
                run_form(f)
            runs = [len(forms["local"][0].fetch(k)[0]) for k in range(K)]
            loads = [forms["local"][0].fetch(k)[1] for k in range(K)]
            same = all(forms["local"][1][k][0].fetch()[1].tobytes() == forms[f][1][k][0].fetch()[1].tobytes()
                       for k in (0, K - 1) for f in ("packed", "zero_copy"))
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "route_runs": runs, "route_loads": loads,
                         "chain_ms": {f: list(both[f]) for f in names}, "router_ms": {f: list(alone[f]) for f in names},
                         "local_against_packed": verdict(both["local"], both["packed"]),
                         "local_against_zero_copy": verdict(both["local"], both["zero_copy"]),
                         "router_local_against_packed": verdict(alone["local"], alone["packed"]),
                         "router_local_against_zero_copy": verdict(alone["local"], alone["zero_copy"]),
                         "resampled_payloads_equal": bool(same)}
            gate.close()
        out["%dx%d" % (nch, K)] = res
        for router, chains in forms.values():
            for rr, st in chains:
                st.close()
                rr.close()
            router.close()
        sq.close()
        del d_rows, keep
    print(json.dumps(out))


def bench_runbits(a, pkg, torch):
    """the A/B of the sign-bit path: burst resampler -> burst stage in the PCM form and in the bits form on the device view one gate
    call left (every call begins every stretch anew, as in bench_runrs), alternating in one process in rotating order; AIS and
    POCSAG on the busy rows, ratio, taps and window of bench_runais / bench_runpocsag; all-open, half-open (a squelch at the median
    window energy) and all-closed"""
    b = pkg.binding
    nch, W, I, D = a.bench_channels, a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runbits_stage", "channels": nch, "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I,
           "decimate": D, "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner,
           "rule": "kept / worse when the means differ by more than 2 standard errors of their difference, else neutral"}
    for proto in ("ais", "pocsag"):
        host = _busy_rows(pkg, nch, n) if proto == "ais" else _busy_pocsag_rows(pkg, nch, n)
        polarity = b.MFM_BITS_POS if proto == "ais" else b.MFM_BITS_NEG
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "half_open": scene["open"]}
        keep, recs = [], {"half_open": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        # a chain of its own per form: a stage's state moves with every call, and the two forms must not see each other's
        rr_p = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rr_b = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        stage = pkg.RunAis if proto == "ais" else pkg.RunPocsag
        st_p, st_b = stage.behind(rr_p), stage.behind(rr_b)
        res = {}
        for name in ("all_open", "half_open", "all_closed"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_pcm():
                rr_p.process_device(*view)
                st_p.process_device(*rr_p.device_view())

            def run_bits():
                rr_b.process_bits_device(*view, polarity)
                st_b.process_bits_device(rr_b.bits_view())

            variants = [("pcm", run_pcm), ("bits", run_bits)]
            for _, fn in variants:
                timed(fn, 3)
            ev_p, ev_b = st_p.fetch(), st_b.fetch()
            got = {v: [] for v, _ in variants}
            for rep_ in range(a.reps):
                k = rep_ % len(variants)
                for vname, fn in variants[k:] + variants[:k]:
                    got[vname].append(timed(fn, a.inner))
            (pm, psd), (bm, bsd) = _stats(got["pcm"]), _stats(got["bits"])
            se = math.sqrt(psd * psd / a.reps + bsd * bsd / a.reps)
            d = bm - pm
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "events_per_call": int(len(ev_p)),
                         "events_identical": bool(ev_p.tobytes() == ev_b.tobytes()), "pcm_ms": pm, "pcm_sd": psd, "bits_ms": bm, "bits_sd": bsd,
                         "bits_over_pcm": bm / pm, "difference_ms": d, "difference_se": se,
                         "verdict": "neutral" if abs(d) <= 2.0 * se else ("kept" if d < 0 else "worse")}
            gate.close()
        out[proto] = res
        for o in (st_p, st_b, rr_p, rr_b, sq):
            o.close()
        del d_rows, keep
    print(json.dumps(out))


def bench_runends(a, pkg, torch):
    """what the stretch-end report costs: each of the three burst stages at 64 and 1024 channels on the half-open mask of the
    stages' own lines (the squelch on the median window energy), the stage's process call alone on the device view one burst
    resampler call left (every call begins every stretch anew, so every call does the same work and a stretch ends behind every
    run that has a successor on its channel).  Report off and report on alternate in one process in rotating order; with
    --runends-parent LIB a third variant calls the same entry of that library (the parent commit's build) on the same buffers,
    which is the figure "off is free" is read from"""
    b = pkg.binding
    W = a.window
    n = 1 << 17
    nw = n // W
    nb = nw * W
    cases = {"ais": (4, 5, np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16), _busy_rows, pkg.RunAis, b.RunaisConfig),
             "pocsag": (4, 5, np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16), _busy_pocsag_rows, pkg.RunPocsag,
                        b.RunPocsagConfig),
             "flex": (16, 25, np.round(pkg.synth.design_lpf(101, 0.45 / 25, 1.0) * 16 * 16384.0).astype(np.int16), _busy_flex_rows, pkg.RunFlex,
                      b.RunFlexConfig)}
    parent = C.CDLL(os.path.abspath(a.runends_parent)) if a.runends_parent else None

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "run_ends_stage", "window": W, "samples_per_channel": nb, "mask": "half_open", "reps": a.reps, "calls_per_rep": a.inner,
           "parent": bool(parent)}
    for stage, (I, D, taps, rows_of, Stage, Config) in cases.items():
        for nch in (64, 1024):
            d_rows = torch.from_numpy(np.ascontiguousarray(rows_of(pkg, nch, n))).cuda()
            rows, in_stride = d_rows.data_ptr(), n
            probe = pkg.Level(nch, n, W, device=0)
            probe.process_device(rows, in_stride, nb)
            thr = int(np.median(probe.fetch()["energy"]))
            probe.close()
            sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
            sq.process_device(rows, in_stride, nb)
            open_share = float(sq.fetch()["open"].astype(bool).mean())
            d_scene, scene_stride, _, _ = sq.device_view()
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, d_scene, scene_stride, nw)
            rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
            rr.process_device(*gate.device_view())
            view = rr.device_view()
            nr_runs = len(rr.fetch()[0])
            off, on = Stage.behind(rr), Stage.behind(rr)
            on.set_end_report(True)
            variants = [("off", lambda: off.process_device(*view)), ("on", lambda: on.process_device(*view))]
            ph = C.c_void_p()
            if parent:
                max_runs, max_out = rr.capacity()
                cfg = Config(b.MFM_ABI_VERSION, 0, nch, max_runs, max_out, 0, 0, 0) if stage == "flex" else \
                    Config(b.MFM_ABI_VERSION, 0, nch, max_runs, max_out, 0, 0)
                create, process = getattr(parent, f"mfm_run{stage}_create"), getattr(parent, f"mfm_run{stage}_process_device")
                process.argtypes = [C.c_void_p] * 5
                assert create(C.byref(ph), C.byref(cfg)) == 0
                variants.insert(0, ("parent", lambda: process(ph, view[0], view[1], view[2], None)))
            for _, fn in variants:
                timed(fn, 3)
            ends = on.fetch_ends()
            got = {v: [] for v, _ in variants}
            for r in range(a.reps):
                k = r % len(variants)
                for vname, fn in variants[k:] + variants[:k]:
                    got[vname].append(timed(fn, a.inner))
            res = {"runs_per_call": nr_runs, "open_share": open_share, "records_per_call": len(ends), "cut_per_call": int((ends["mode"] != 0).sum())}
            for vname in got:
                res[vname + "_ms"], res[vname + "_sd"] = _stats(got[vname])
            (fm, fsd), (nm, nsd) = _stats(got["off"]), _stats(got["on"])
            res["on_over_off"] = nm / fm
            res["on_over_off_se"] = nm / fm * math.sqrt(fsd * fsd / a.reps / (fm * fm) + nsd * nsd / a.reps / (nm * nm))
            if parent:   # tools/exp/ab.py's rule: worse only beyond two standard errors of the difference of the means
                pm, psd = _stats(got["parent"])
                res["off_minus_parent_ms"], res["two_se"] = fm - pm, 2.0 * math.sqrt(fsd * fsd / a.reps + psd * psd / a.reps)
                res["off_vs_parent"] = "worse" if fm - pm > res["two_se"] else "kept" if pm - fm > res["two_se"] else "neutral"
                torch.cuda.synchronize()
                getattr(parent, f"mfm_run{stage}_destroy")(C.byref(ph))
            out[f"{stage}_{nch}"] = res
            for o in (on, off, rr, gate, sq):
                o.close()
            del d_rows
    print(json.dumps(out))


def bench_runends_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runends needs the GPU: there is no CPU path to time")
    bench_runends(a, pkg, torch)


def bench_runbits_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runbits needs the GPU: there is no CPU path to time")
    bench_runbits(a, pkg, torch)


def bench_runroute_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runroute needs the GPU: there is no CPU path to time")
    bench_runroute(a, pkg, torch)


def bench_runroute_pack_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runroute-pack needs the GPU: there is no CPU path to time")
    bench_runroute_pack(a, pkg, torch)


def bench_runroute_local_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runroute-local needs the GPU: there is no CPU path to time")
    bench_runroute_local(a, pkg, torch)


def bench_runflex_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runflex needs the GPU: there is no CPU path to time")
    bench_runflex(a, pkg, torch)


def bench_runmm(a, pkg, torch):
    """burst resampler -> burst Mueller-Muller stage on the device view one gate call left (every call begins every stretch anew,
    as in bench_runrs, so every call does the same work) against mfm_resampler (v_dot2 form) -> mfm_mm on the full rows; the two
    chains alternate in one process in rotating order.  The decisions of a call's first runs are compared with the host twin's"""
    b = pkg.binding
    W, I, D = a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)
    spb = float(np.float32(38400.0) / np.float32(1200.0))   # the busy rows' 1200-baud transmissions behind the 4/5 resampler
    mm = dict(MM_DEFAULTS, spb=spb)
    emin, emax = float(np.float32(spb) - np.float32(mm["margin"])), float(np.float32(spb) + np.float32(mm["margin"]))

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runmm_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I, "decimate": D,
           "taps": int(taps.size), "reps": a.reps, "calls_per_rep": a.inner, "samples_per_bit": spb, "kw": mm["kw"], "km": mm["km"],
           "margin": mm["margin"], "staging_unit": b.RUNMM_STAGING_UNIT}
    sample_ok, sample_decisions = True, 0
    for nch in (64, 1024):
        host = _busy_pocsag_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
        keep, recs = [], {"scene": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        plain = pkg.Resampler(nch, taps, I, D, nb, device=0, force_dot2=True)
        pm_ = pkg.MuellerMuller(nch, mm["kw"], mm["km"], spb, emin, emax, plain.max_out(), device=0)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rm = pkg.RunMm.behind(rr, spb, mm["kw"], mm["km"], margin=mm["margin"])

        def run_plain():
            yptr, ystride, ny = plain.process_device(rows, in_stride, nb)
            pm_.process_device(yptr, ystride, ny)

        res = {}
        for name in ("all_closed", "scene", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_burst():
                rr.process_device(*view)
                rm.process_device(*rr.device_view())

            def run_burst_rs():
                rr.process_device(*view)

            def run_plain_rs():
                plain.process_device(rows, in_stride, nb)

            variants = [("burst", run_burst), ("plain", run_plain), ("burst_rs", run_burst_rs), ("plain_rs", run_plain_rs)]
            for _, fn in variants:
                timed(fn, 3)
            run_burst()
            mruns, decs = rm.fetch()
            # a sample against the twin: the call's first runs (each begins its stretch, so each stands alone)
            runs, payload = rr.fetch()
            k = 0
            while k < min(len(runs), 6) and int(runs["out_offset"][k]) + int(runs["nr_out"][k]) <= 1 << 20:
                k += 1
            if k:
                assert (runs["flags"][:k] & 1).all()
                wr, wd = b.hosttwin_runmm_call(b.hosttwin_runmm_state(nch), runs[:k], payload[:int(runs["out_offset"][k - 1]) + int(runs["nr_out"][k - 1])],
                                               spb, mm["kw"], mm["km"], margin=mm["margin"])
                sample_ok = sample_ok and mruns[:k].tobytes() == wr.tobytes() and decs[:wd.size].tobytes() == wd.tobytes()
                sample_decisions += int(wd.size)
            got_t = {v: [] for v, _ in variants}
            for rep_ in range(a.reps):
                j = rep_ % len(variants)
                for vname, fn in variants[j:] + variants[:j]:
                    got_t[vname].append(timed(fn, a.inner))
            (bm, bsd), (pm, psd) = _stats(got_t["burst"]), _stats(got_t["plain"])
            (brm, brsd), (prm, prsd) = _stats(got_t["burst_rs"]), _stats(got_t["plain_rs"])
            ratio = bm / pm
            ratio_se = ratio * math.sqrt(bsd * bsd / a.reps / (bm * bm) + psd * psd / a.reps / (pm * pm))
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(len(runs)),
                         "longest_run_out": int(runs["nr_out"].max()) if len(runs) else 0, "decisions_per_call": int(decs.size),
                         "burst_ms": bm, "burst_sd": bsd, "plain_ms": pm, "plain_sd": psd, "burst_over_plain": ratio,
                         "burst_over_plain_se": ratio_se, "burst_resampler_ms": brm, "burst_resampler_sd": brsd,
                         "plain_resampler_ms": prm, "plain_resampler_sd": prsd, "burst_mm_ms": bm - brm, "plain_mm_ms": pm - prm}
            gate.close()
        out["channels_%d" % nch] = res
        for o in (rm, rr, pm_, plain, sq):
            o.close()
        del d_rows, keep
    out["sample_equals_twin"] = bool(sample_ok)
    out["sample_decisions"] = int(sample_decisions)
    print(json.dumps(out))


def bench_runsync(a, pkg, torch):
    """burst resampler -> burst Mueller-Muller stage with and without the burst sync stage behind it, on the device view one gate
    call left (the masks and shapes of bench_runmm); the variants alternate in one process in rotating order.  The yardstick is the
    Mueller-Muller stage's own call on the same mask: chain with it minus the resampler alone.  The events of a call are compared
    with the host twin's on the decisions fetched"""
    b = pkg.binding
    W, I, D = a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)
    spb = float(np.float32(38400.0) / np.float32(1200.0))
    mm = dict(MM_DEFAULTS, spb=spb)
    words = [0x7CD215D8, 0xA6C6AAAA, 0x870C78F3, 0xB0684E97]   # POCSAG's sync word and three more, as FLEX's would stand beside it

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runsync_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I, "decimate": D,
           "reps": a.reps, "calls_per_rep": a.inner, "samples_per_bit": spb, "words": ["%08x" % w for w in words], "max_distance": 3,
           "either": True, "segment": b.RUNSYNC_SEGMENT}
    twin_ok = True
    for nch in (64, 1024):
        host = _busy_pocsag_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
        keep, recs = [], {"scene": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rm = pkg.RunMm.behind(rr, spb, mm["kw"], mm["km"], margin=mm["margin"])
        rs = pkg.RunSync.behind(rm, words, max_distance=3, either=True)
        res = {}
        for name in ("all_closed", "scene", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_rs():
                rr.process_device(*view)

            def run_mm():
                rr.process_device(*view)
                rm.process_device(*rr.device_view())

            def run_sync():
                rr.process_device(*view)
                rm.process_device(*rr.device_view())
                rs.process_device(*rm.device_view())

            variants = [("sync", run_sync), ("mm", run_mm), ("rs", run_rs)]
            for _, fn in variants:
                timed(fn, 3)
            run_sync()
            sruns, sbits, sev = rs.fetch()
            mruns, decs = rm.fetch()
            wr, wb, we = b.hosttwin_runsync_call(b.hosttwin_runsync_state(nch), mruns, decs, words, max_distance=3, either=True)
            twin_ok = twin_ok and sruns.tobytes() == wr.tobytes() and sbits.tobytes() == wb.tobytes() and sev.tobytes() == we.tobytes()
            got_t = {v: [] for v, _ in variants}
            for rep_ in range(a.reps):
                j = rep_ % len(variants)
                for vname, fn in variants[j:] + variants[:j]:
                    got_t[vname].append(timed(fn, a.inner))
            (sm, ssd), (mmm, msd), (rm_, rsd) = _stats(got_t["sync"]), _stats(got_t["mm"]), _stats(got_t["rs"])
            diff, diff_se = sm - mmm, math.sqrt((ssd * ssd + msd * msd) / a.reps)
            mm_call = mmm - rm_
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(len(mruns)), "decisions_per_call": int(decs.size),
                         "events_per_call": int(sev.size), "chain_with_sync_ms": sm, "chain_with_sync_sd": ssd, "chain_ms": mmm, "chain_sd": msd,
                         "resampler_ms": rm_, "resampler_sd": rsd, "sync_ms": diff, "sync_se": diff_se,
                         "verdict": "costs" if diff > 2 * diff_se else "neutral" if abs(diff) <= 2 * diff_se else "faster",
                         "mm_call_ms": mm_call, "sync_over_mm_call": diff / mm_call if mm_call > 0 else None}
            gate.close()
        out["channels_%d" % nch] = res
        for o in (rs, rm, rr, sq):
            o.close()
        del d_rows, keep
    out["equals_twin"] = bool(twin_ok)
    print(json.dumps(out))


def bench_runbatch(a, pkg, torch):
    """burst resampler -> burst Mueller-Muller -> burst sync with and without the burst batch stage behind it, on the device view
    one gate call left (the masks and shapes of bench_runsync); the variants alternate in one process in rotating order.  The batch
    stage's cost is the difference of the two chains, beside the sync stage's, measured the same way against the chain without it.
    The events of a call are compared with the host twin's on the sync stage's result fetched"""
    b = pkg.binding
    W, I, D = a.window, 4, 5
    n = 1 << 17
    nw = n // W
    nb = nw * W
    taps = np.round(pkg.synth.design_lpf(41, 0.45 / 5, 1.0) * 4 * 16384.0).astype(np.int16)
    spb = float(np.float32(38400.0) / np.float32(1200.0))
    mm = dict(MM_DEFAULTS, spb=spb)
    words = [0x7CD215D8, 0xA6C6AAAA, 0x870C78F3, 0xB0684E97]   # as bench_runsync

    def timed(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / inner

    out = {"bench": "runbatch_stage", "window": W, "samples_per_channel": nb, "windows_per_channel": nw, "interpolate": I, "decimate": D,
           "reps": a.reps, "calls_per_rep": a.inner, "samples_per_bit": spb, "words": ["%08x" % w for w in words], "max_distance": 3,
           "either": True, "keep_distance": 4, "frame": b.RUNBATCH_FRAME}
    twin_ok = True
    for nch in (64, 1024):
        host = _busy_pocsag_rows(pkg, nch, n)
        d_rows = torch.from_numpy(np.ascontiguousarray(host)).cuda()
        rows, in_stride = d_rows.data_ptr(), n
        probe = pkg.Level(nch, n, W, device=0)
        probe.process_device(rows, in_stride, nb)
        thr = int(np.median(probe.fetch()["energy"]))
        probe.close()
        sq = pkg.Level(nch, n, W, sense=b.MFM_LEVEL_OPEN_ABOVE, open_thr=thr, close_thr=thr, device=0)
        sq.process_device(rows, in_stride, nb)
        scene = sq.fetch()
        d_scene, scene_stride, _, _ = sq.device_view()
        masks = {"all_closed": np.zeros((nch, nw), np.uint32), "all_open": np.ones((nch, nw), np.uint32), "scene": scene["open"]}
        keep, recs = [], {"scene": (d_scene, scene_stride)}
        for name in ("all_closed", "all_open"):
            r = np.zeros((nch, nw), b.LEVEL_RECORD_DTYPE)
            r["window"] = np.arange(nw, dtype=np.uint64)[None, :]
            r["open"] = masks[name]
            t = torch.from_numpy(r.view(np.uint8).reshape(-1).copy()).cuda()
            keep.append(t)
            recs[name] = (t.data_ptr(), nw)
        rr = pkg.RunResampler(nch, taps, I, D, W, max_in_samples=n, device=0)
        rm = pkg.RunMm.behind(rr, spb, mm["kw"], mm["km"], margin=mm["margin"])
        rs = pkg.RunSync.behind(rm, words, max_distance=3, either=True)
        rb = pkg.RunBatch.behind(rs, keep_distance=4)
        res = {}
        for name in ("all_closed", "scene", "all_open"):
            gate = pkg.Gate(nch, n, W, device=0)
            gate.process_device(rows, in_stride, nb, recs[name][0], recs[name][1], nw)
            view = gate.device_view()

            def run_mm():
                rr.process_device(*view)
                rm.process_device(*rr.device_view())

            def run_sync():
                run_mm()
                rs.process_device(*rm.device_view())

            def run_batch():
                run_sync()
                rb.process_device(*rs.device_view())

            variants = [("batch", run_batch), ("sync", run_sync), ("mm", run_mm)]
            for _, fn in variants:
                timed(fn, 3)
            run_batch()
            bev = rb.fetch()
            sruns, sbits, sev = rs.fetch()
            want = b.hosttwin_runbatch_call(b.hosttwin_runbatch_state(nch), sruns, sbits, sev, words, keep_distance=4)
            twin_ok = twin_ok and bev.tobytes() == want.tobytes()
            got_t = {v: [] for v, _ in variants}
            for rep_ in range(a.reps):
                j = rep_ % len(variants)
                for vname, fn in variants[j:] + variants[:j]:
                    got_t[vname].append(timed(fn, a.inner))
            (bm, bsd), (sm, ssd), (mmm, msd) = _stats(got_t["batch"]), _stats(got_t["sync"]), _stats(got_t["mm"])
            diff, diff_se = bm - sm, math.sqrt((bsd * bsd + ssd * ssd) / a.reps)
            sdiff, sdiff_se = sm - mmm, math.sqrt((ssd * ssd + msd * msd) / a.reps)
            res[name] = {"open_share": float(masks[name].astype(bool).mean()), "runs": int(len(sruns)),
                         "decisions_per_call": int(sruns["nr_dec"].astype(np.uint64).sum()), "sync_events_per_call": int(sev.size),
                         "events_per_call": int(bev.size), "batches_per_call": int((bev["type"] == 2).sum()),
                         "chain_with_batch_ms": bm, "chain_with_batch_sd": bsd, "chain_ms": sm, "chain_sd": ssd, "batch_ms": diff,
                         "batch_se": diff_se,
                         "verdict": "costs" if diff > 2 * diff_se else "neutral" if abs(diff) <= 2 * diff_se else "faster",
                         "sync_ms": sdiff, "sync_se": sdiff_se, "batch_over_sync": diff / sdiff if sdiff > 0 else None}
            gate.close()
        out["channels_%d" % nch] = res
        for o in (rb, rs, rm, rr, sq):
            o.close()
        del d_rows, keep
    out["equals_twin"] = bool(twin_ok)
    print(json.dumps(out))


def bench_runbatch_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runbatch needs the GPU: there is no CPU path to time")
    bench_runbatch(a, pkg, torch)


def bench_runsync_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runsync needs the GPU: there is no CPU path to time")
    bench_runsync(a, pkg, torch)


def bench_runmm_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runmm needs the GPU: there is no CPU path to time")
    bench_runmm(a, pkg, torch)


def bench_runpocsag_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runpocsag needs the GPU: there is no CPU path to time")
    bench_runpocsag(a, pkg, torch)


def bench_runais_alone(a):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("--bench-runais needs the GPU: there is no CPU path to time")
    bench_runais(a, pkg, torch)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config")
    ap.add_argument("--input")
    ap.add_argument("--format", choices=["cs16", "cs8", "cu8"], default="cs16")
    ap.add_argument("--form", choices=["pcm", "iq"], default="pcm")
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--metric", choices=["energy", "diff"], default="energy")
    ap.add_argument("--sense", choices=["above", "below"], default=None)
    ap.add_argument("--open-thr", type=int, default=0)
    ap.add_argument("--close-thr", type=int, default=None)
    ap.add_argument("--hang", type=int, default=0)
    ap.add_argument("--floor-windows", type=int, default=None, help="M: the adaptive squelch on the floor of the last M windows")
    ap.add_argument("--open-ratio", type=float, default=None, help="opens at this ratio to the floor (with --floor-windows)")
    ap.add_argument("--close-ratio", type=float, default=None, help="a window is bad beyond this ratio to the floor (with --floor-windows)")
    ap.add_argument("--warmup", type=int, default=None, help="windows after the start that open nothing (with --floor-windows)")
    ap.add_argument("--block", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--summary", action="store_true")
    ap.add_argument("--gate-out", default=None)
    ap.add_argument("--gate-preroll", default="0", help="pre-roll windows of the gate; with --bench one or several, as 0,1,4")
    ap.add_argument("--gate-resample", default=None, help="I/D: resample the gate's runs on the device (with --gate-out, --form pcm)")
    ap.add_argument("--resample-taps", default=None, help="JSON file whose lpfCoeffs are the resampler's taps")
    ap.add_argument("--gate-dc-pole", type=float, default=None,
                    help="the burst resampler's DC blocker with this pole, a fresh one per stretch (with --gate-resample, not with --gate-bits)")
    ap.add_argument("--gate-ais", action="store_true", help="demodulate AIS on the resampled runs on the device (with --gate-resample)")
    ap.add_argument("--gate-pocsag", action="store_true", help="demodulate POCSAG on the resampled runs on the device (with --gate-resample)")
    ap.add_argument("--gate-flex", action="store_true", help="decode FLEX on the resampled runs on the device (with --gate-resample to 16 000 Hz)")
    ap.add_argument("--gate-mm", default=None, metavar="SPB[,KW,KM,MARGIN]",
                    help="Mueller-Muller clock recovery on the resampled runs on the device (with --gate-resample): the decisions of every run")
    ap.add_argument("--gate-sync", default=None, metavar="WORD[,WORD...][/DIST][,either]",
                    help="with --gate-mm: the burst sync stage behind it, sync words in the decisions; one line per event in sync.jsonl")
    ap.add_argument("--gate-batch", default=None, nargs="?", const="", metavar="KEEP[,BAUD]",
                    help="with --gate-sync: the burst batch stage behind it, POCSAG batches behind the sync events; one line per event in "
                         "batch.jsonl and the pages in pages.jsonl")
    ap.add_argument("--gate-bits", action="store_true",
                    help="with --gate-ais or --gate-pocsag: sign bits instead of PCM between the burst resampler and the stage")
    ap.add_argument("--gate-ends", action="store_true",
                    help="with --gate-ais, --gate-pocsag, --gate-flex or --gate-route: one line per stretch in ends.jsonl, how it ended and what the squelch cut")
    ap.add_argument("--gate-route", default=None,
                    help="JSON file of routes: one gate feeds a burst chain per protocol through the run router (with --gate-out, --form pcm)")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-level-adaptive", action="store_true", help="the level_adaptive_stage line of --bench alone")
    ap.add_argument("--bench-floor-windows", default="64,1,1024", help="the M's of the level_adaptive_stage line; the first against the fixed path")
    ap.add_argument("--bench-runrs", action="store_true", help="the runrs_stage and runrs_dc_stage lines of --bench alone")
    ap.add_argument("--bench-runais", action="store_true", help="the runais_stage line of --bench alone")
    ap.add_argument("--bench-runpocsag", action="store_true", help="the runpocsag_stage line of --bench alone")
    ap.add_argument("--bench-runflex", action="store_true", help="the runflex_stage line alone")
    ap.add_argument("--bench-runmm", action="store_true",
                    help="the runmm_stage line: burst resampler -> burst Mueller-Muller against the full-row chain at 64 and 1024 channels")
    ap.add_argument("--bench-runsync", action="store_true",
                    help="the runsync_stage line: the burst Mueller-Muller chain with and without the burst sync stage at 64 and 1024 channels")
    ap.add_argument("--bench-runbatch", action="store_true",
                    help="the runbatch_stage line: the burst sync chain with and without the burst batch stage at 64 and 1024 channels")
    ap.add_argument("--bench-runbits", action="store_true", help="the runbits_stage line of --bench alone")
    ap.add_argument("--bench-runroute", action="store_true", help="the runroute_stage line alone: the run router at 64 and 1024 channels")
    ap.add_argument("--bench-runroute-pack", action="store_true",
                    help="the runroute_pack_stage line: packed routes against zero-copy routes at 64 and 1024 channels, 2 and 8 routes")
    ap.add_argument("--pack-only", default=None, metavar="SHAPE/MASK",
                    help="with --bench-runroute-pack: one case alone, e.g. 1024x2/half_open, for a kernel trace of its own")
    ap.add_argument("--bench-runroute-local", action="store_true",
                    help="the runroute_local_stage line: zero-copy, packed and local routes at 64 and 1024 channels, 2 and 8 routes")
    ap.add_argument("--bench-runends", action="store_true",
                    help="the run_ends_stage line: the three burst stages at 64 and 1024 channels, the stretch-end report off and on")
    ap.add_argument("--runends-parent", default=None, metavar="LIB",
                    help="with --bench-runends: a third variant, the same stage entry of this library (the parent commit's build)")
    ap.add_argument("--bench-channels", type=int, default=64)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    if a.bench_runais:
        return bench_runais_alone(a)
    if a.bench_runpocsag:
        return bench_runpocsag_alone(a)
    if a.bench_runflex:
        return bench_runflex_alone(a)
    if a.bench_runmm:
        return bench_runmm_alone(a)
    if a.bench_runsync:
        return bench_runsync_alone(a)
    if a.bench_runbatch:
        return bench_runbatch_alone(a)
    if a.bench_runends:
        return bench_runends_alone(a)
    if a.bench_runbits:
        return bench_runbits_alone(a)
    if a.bench_runroute:
        return bench_runroute_alone(a)
    if a.bench_runroute_pack:
        return bench_runroute_pack_alone(a)
    if a.bench_runroute_local:
        return bench_runroute_local_alone(a)
    if a.bench or a.bench_runrs or a.bench_level_adaptive:
        return bench(a)
    if not a.config or not a.input:
        ap.error("--config and --input are required (or --bench)")
    if (a.floor_windows is None) != (a.open_ratio is None) or (a.floor_windows is None) != (a.close_ratio is None):
        raise SystemExit("--floor-windows, --open-ratio and --close-ratio go together: the adaptive squelch needs all three")
    if a.warmup is not None and a.floor_windows is None:
        raise SystemExit("--warmup needs --floor-windows: it is the adaptive squelch's warm-up")
    if a.gate_batch is not None:
        if not a.gate_sync:
            raise SystemExit("--gate-batch needs --gate-sync: the burst batch stage takes the burst sync stage's events and bits")
        parse_gate_batch(a.gate_batch)
    if a.gate_sync:
        if not a.gate_mm:
            raise SystemExit("--gate-sync needs --gate-mm: the burst sync stage takes the burst Mueller-Muller stage's decisions")
        parse_gate_sync(a.gate_sync)
    if a.gate_mm:
        if a.gate_route:
            raise SystemExit("--gate-route excludes --gate-mm: a route of stage mm names its own loop")
        if not a.gate_resample:
            raise SystemExit("--gate-mm needs --gate-resample: the burst Mueller-Muller stage takes the burst resampler's runs")
        if a.gate_ais or a.gate_pocsag or a.gate_flex:
            raise SystemExit("--gate-mm, --gate-flex, --gate-pocsag and --gate-ais exclude each other: one stage reads the burst resampler's runs")
        if a.gate_bits:
            raise SystemExit("--gate-mm and --gate-bits exclude each other: the burst Mueller-Muller stage reads PCM values, not sign bits")
        if a.gate_ends:
            raise SystemExit("--gate-mm and --gate-ends exclude each other: a decision never looks ahead, so nothing is cut when a stretch ends")
        parse_gate_mm(a.gate_mm)
    if a.gate_route and (a.gate_resample or a.gate_ais or a.gate_pocsag or a.gate_flex or a.gate_bits or a.gate_dc_pole is not None):
        raise SystemExit("--gate-route excludes --gate-resample, --gate-ais, --gate-pocsag, --gate-flex, --gate-bits and --gate-dc-pole: "
                         "every route names its own resampler and stage")
    if a.gate_route and (not a.gate_out or a.form != "pcm"):
        raise SystemExit("--gate-route needs --gate-out and --form pcm: the burst resamplers take PCM payloads only")
    if a.gate_route:
        read_routes(a.gate_route, len(read_config(a.config)[4]))   # what is wrong with FILE ends the run before anything is set up
    if a.gate_ends and not (a.gate_ais or a.gate_pocsag or a.gate_flex or a.gate_route):
        raise SystemExit("--gate-ends needs --gate-ais, --gate-pocsag, --gate-flex or --gate-route: it is the burst stage's stretch-end report")
    if a.gate_flex and not a.gate_resample:
        raise SystemExit("--gate-flex needs --gate-resample: the burst FLEX stage takes the burst resampler's runs")
    if a.gate_flex and (a.gate_ais or a.gate_pocsag):
        raise SystemExit("--gate-flex, --gate-pocsag and --gate-ais exclude each other: one stage reads the burst resampler's runs")
    if a.gate_dc_pole is not None and not a.gate_resample:
        raise SystemExit("--gate-dc-pole needs --gate-resample: it is the burst resampler's DC blocker")
    if a.gate_dc_pole is not None and a.gate_bits:
        raise SystemExit("--gate-dc-pole and --gate-bits exclude each other: the DC blocker filters the PCM the sign bits would be taken from")
    if a.gate_bits and a.gate_flex:
        raise SystemExit("--gate-bits and --gate-flex exclude each other: the burst FLEX stage reads PCM values, not sign bits")
    if a.gate_bits and a.gate_ais == a.gate_pocsag:
        raise SystemExit("--gate-bits needs --gate-ais or --gate-pocsag (one of them): it is the path between the burst resampler and that stage")
    scan(a)


if __name__ == "__main__":
    main()
