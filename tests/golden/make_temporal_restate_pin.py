#!/usr/bin/env python3
"""Writes tests/golden/temporal_restate_pin.json: SHA-256 digests of every output array of the numpy restatements of the three
temporal merges (tests/temporal_restate.py, temporal_rectify_restate.py, temporal_cascade_restate.py) on their own synthetic frames,
and their `info` branch counts. The restatements are the oracle of the device and host forms; the pin is what lets the oracle itself
be rewritten: tests/test_temporal_restate_pin.py recomputes the digests and compares. NaNs are canonicalised before hashing (the
definitions do not fix a payload). Needs numpy only; run after a change that is MEANT to change what a restatement computes:

    python tests/golden/make_temporal_restate_pin.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
PIN = os.path.join(HERE, "temporal_restate_pin.json")

SIZES = ((37, 23), (64, 4), (8, 8), (1, 1))
SEED = 0
MIN_TAPS, GAMMA = 8, 3.0  # the defaults of TwkTemporalRectify
RECTIFY = ((1, GAMMA), (3, GAMMA), (4, GAMMA), (3, 0.0))  # (radius, gamma)
LAYERS = (2, 6, 8)


def digest(a):
    """SHA-256 of dtype, shape and bytes of `a`, every NaN replaced by the quiet NaN of its format"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = np.where(np.isnan(a), a.dtype.type(np.nan), a).astype(a.dtype)
    h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode())
    h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def compute():
    """{"digests": {case: sha256}, "info": {case: branch counts}}"""
    import temporal_cascade_restate as tc
    import temporal_rectify_restate as tr
    import temporal_restate as t

    digests, infos = {}, {}

    def record(case, names, arrays, info=None):
        assert len(names) == len(arrays), case
        for name, a in zip(names, arrays):
            digests[f"{case}/{name}"] = digest(a)
        if info is not None:
            infos[case] = {k: int(v) for k, v in sorted(info.items())}

    for width, height in SIZES:
        size = f"{width}x{height}"
        if width * height > tc._SPECIALS:  # synthetic_frames plants 56 special pixels
            (cur, mc, g), history, cam, max_history, tolerance = t.synthetic_frames(width, height, SEED)
            info = {}
            record(f"restate_temporal/{size}", ("colour", "moments", "took"), t.restate_temporal(cur, mc, g, history, cam, max_history, tolerance, info), info)
            record(f"restate_temporal/{size}/no_history", ("colour", "moments", "took"), t.restate_temporal(cur, mc, g, None, cam, max_history, tolerance))
        (cur, mc, g), history, cam, max_history, tolerance = tr.rectify_frames(width, height, SEED)
        record(f"restate_temporal/rectify_frames/{size}", ("colour", "moments", "took"), t.restate_temporal(cur, mc, g, history, cam, max_history, tolerance))
        h, hmean, hm2, hn, took = tr.reproject(cur, mc, g, history, cam, max_history, tolerance)
        record(f"reproject/{size}", ("h", "hmean", "hM2", "hn", "took"), (h, hmean, hm2, hn, took))
        record(f"reproject/{size}/no_history", ("h", "hmean", "hM2", "hn", "took"), tr.reproject(cur, mc, g, None, cam, max_history, tolerance))
        for radius, gamma in RECTIFY:
            case = f"{size}/radius{radius}_gamma{gamma:g}"
            info = {}
            record(f"trust_of/{case}", ("trust",), (tr.trust_of(mc, g, hmean, hn, radius, MIN_TAPS, gamma, info),), info)
            info = {}
            record(f"restate_rectify/{case}", ("colour", "moments", "trust", "merged"), tr.restate_rectify(cur, mc, g, history, cam, max_history, tolerance, radius, MIN_TAPS, gamma, info), info)
            with np.errstate(over="ignore", invalid="ignore"):
                raws = (("f32", cur), ("f16", cur.astype(np.float16)))
            for fmt, raw in raws:
                record(f"expect_rectify/{case}/{fmt}", ("colourOut", "historyOut", "momentsOut", "trustOut", "merged"),
                       tr.expect_rectify(raw, mc, g, history, cam, max_history, tolerance, radius, MIN_TAPS, gamma))
        for K in LAYERS:
            case = f"{size}/K{K}"
            Lc, lg, lhistory, lcam, max_history, tolerance, _ = tc.synthetic_layers(width, height, K, SEED)
            info = {}
            record(f"restate_temporal_cascade/{case}", ("layers", "took"), tc.restate_temporal_cascade(Lc, lg, lhistory, lcam, max_history, tolerance, info), info)
            record(f"restate_temporal_cascade/{case}/no_history", ("layers", "took"), tc.restate_temporal_cascade(Lc, lg, None, lcam, max_history, tolerance))
            rng = np.random.default_rng(SEED + 9)
            trust = rng.uniform(0.0, 1.0, (height, width)).astype(np.float32)
            trust[rng.uniform(size=trust.shape) < 0.1] = 0
            trust[rng.uniform(size=trust.shape) < 0.1] = 1
            record(f"restate_temporal_cascade_trusted/{case}", ("layers", "took", "hn"), tr.restate_temporal_cascade_trusted(Lc, lg, lhistory, lcam, max_history, tolerance, trust))
            record(f"restate_temporal_cascade_trusted/{case}/no_history", ("layers", "took", "hn"), tr.restate_temporal_cascade_trusted(Lc, lg, None, lcam, max_history, tolerance, trust))
    return {"digests": digests, "info": infos}


if __name__ == "__main__":
    pin = compute()
    with open(PIN, "w") as f:
        json.dump(pin, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{PIN}: {len(pin['digests'])} digests, {len(pin['info'])} sets of branch counts")
