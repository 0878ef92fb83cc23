"""CPU: the numpy restatements of the three temporal merges (tests/temporal_restate.py, temporal_rectify_restate.py,
temporal_cascade_restate.py) still compute what they computed when tests/golden/temporal_restate_pin.json was written: every output
array of restate_temporal, reproject, trust_of, restate_rectify, expect_rectify, restate_temporal_cascade and
restate_temporal_cascade_trusted on their synthetic frames, by SHA-256 (NaNs canonicalised), and every branch count. The
restatements are the oracle of the device and host forms, which the other tests compare with them bit for bit; this pins the oracle
itself, so that it can be rewritten together with the code it judges. No GPU, no library."""
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_temporal_restate_pin", os.path.join(GOLDEN, "make_temporal_restate_pin.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_restatements_compute_what_the_pin_recorded():
    generator = _generator()
    with open(generator.PIN) as f:
        pin = json.load(f)
    now = generator.compute()
    assert sorted(now["digests"]) == sorted(pin["digests"]), "the cases of the generator are the cases of the fixture"
    assert len(pin["digests"]) > 400 and len(pin["info"]) > 40
    differing = [case for case in sorted(pin["digests"]) if now["digests"][case] != pin["digests"][case]]
    assert not differing, f"{len(differing)} of {len(pin['digests'])} arrays differ from the pin, first {differing[:6]}"
    assert now["info"] == pin["info"], [case for case in pin["info"] if now["info"].get(case) != pin["info"][case]][:6]
