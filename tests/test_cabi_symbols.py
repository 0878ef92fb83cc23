"""CPU: libtweeker_hip.so loads without a GPU and exports exactly the functions include/tweeker_hip.h declares."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


def _header_functions():
    text = open(os.path.join(ROOT, "include", "tweeker_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(twk_[a-z0-9_]+)\s*\(", text)))


def test_header_python_binding_and_library_agree(twk):
    from tweeker_raytracer_amd import _lib
    declared = _header_functions()
    assert len(declared) >= 50
    assert sorted(_lib.SYMBOLS) == declared, set(_lib.SYMBOLS) ^ set(declared)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (twk_[a-z0-9_]+)$", out, flags=re.M)))
    assert exported == declared, set(exported) ^ set(declared)
    for name in declared:
        assert getattr(_lib.lib, name) is not None
    assert _lib.lib.twk_abi_version() == 9


def test_no_gpu_means_loud_failure_not_fallback(twk):
    """Without a HIP device twk_device_create must fail with TWK_ERROR_NO_DEVICE (there is no CPU path)."""
    try:
        n = twk.device_count()
    except twk.TwkError as e:
        assert e.code == 2
        n = 0
    if n > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(twk.TwkError) as e:
        twk.Device(ordinal=0)
    assert e.value.code == 2 and "no CPU path" in str(e.value)


def test_product_does_not_link_or_import_the_oracle():
    from tweeker_raytracer_amd import _lib
    needed = subprocess.run(["readelf", "-d", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "oracle" not in needed
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tweeker_raytracer_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")) or f == "Makefile":
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "orc_" not in src and "liboracle" not in src and "from oracle" not in src and "import oracle" not in src, os.path.join(dirpath, f)


def test_every_entry_point_is_a_function_try_block():
    """No C++ exception may cross the extern "C" boundary (the reference throws std::runtime_error, inc/CheckMacros.h:38-80;
    a C caller cannot catch it): every definition of an `int twk_*(...)` entry point in the files that hold them (every
    csrc/*.hip and host/host_cabi.cpp) is a function-try-block ending in TWK_CATCH("<its own name>"), except the few one-liners
    that cannot throw; and every declared entry point is defined exactly once across them."""
    cannot_throw = {"twk_abi_version", "twk_app_destroy"}  # return a constant / delete a pointer
    csrc = os.path.join(ROOT, "tweeker_raytracer_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip")) + ["host/host_cabi.cpp"]
    assert len(files) > 2
    seen = []
    for rel in files:
        text = open(os.path.join(csrc, rel)).read()
        for m in re.finditer(r"^int (twk_[a-z0-9_]+)\s*\(([^)]*)\)\s*\n(\S+)", text, flags=re.M):
            name, following = m.group(1), m.group(3)
            seen.append(name)
            if name in cannot_throw:
                continue
            assert following == "try", f"{rel}: {name} is not a function-try-block"
            assert f'TWK_CATCH("{name}")' in text, f"{rel}: {name} has no TWK_CATCH of its own"
        for m in re.finditer(r"^int (twk_[a-z0-9_]+)\s*\([^)]*\)\s*\{", text, flags=re.M):  # one-line definitions
            seen.append(m.group(1))
            assert m.group(1) in cannot_throw, f"{rel}: {m.group(1)} is defined without a try block"
    declared = set(_header_functions()) - {"twk_last_error"}
    assert declared <= set(seen), declared - set(seen)
    for name in declared:
        assert seen.count(name) == 1, f"{name} is defined {seen.count(name)} times"


def test_bench_carries_pmc_traffic_only_for_the_matching_launch_size():
    """bench.py reports roofline.traffic (HBM-side bytes of the traversal kernel, rocprofv3 --pmc) only from a committed
    record taken at THIS run's steps / batch depth / resolution / tessellation: the driver's `--steps 20 --warmup 5` line and
    the default 64-step line each find their own record, anything else gets null with the reason."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("twk_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rec, name = bench.pick_pmc_record(20, 20, (1920, 1080))
    # the newest record (by name: rNN_...) of the matching launch size wins: round 5's, taken on the round's final kernels
    assert rec is not None and name == "r05_trace_hbm_traffic_s20.json" and rec["steps"] == 20 and rec["hbm_bytes_per_launch"] > 1e9
    rec64, name64 = bench.pick_pmc_record(64, 64, (1920, 1080))
    assert rec64 is not None and name64 == "r05_trace_hbm_traffic_s64.json" and rec64["hbm_bytes_per_launch"] > 2.5 * rec["hbm_bytes_per_launch"]
    # the shade kernel has records of its own (roofline.shade), and they carry the uncapped issue ratio; since the class-ordered
    # windows (round 5) more than half of the lanes are active per vector instruction (the review's threshold: 0.55; 0.37 before)
    shade, shade_name = bench.pick_pmc_record(20, 20, (1920, 1080), kernel="shade")
    assert shade is not None and shade_name == "r05_shade_hbm_traffic_s20.json" and shade["valu_issue_ratio_uncapped_4_clock_model"] > 0.5 and shade["valu_lane_utilisation"] >= 0.55
    big, _ = bench.pick_pmc_record(32, 32, (1920, 1080), 2800)
    assert big is not None and big["sphere_tess"] == 2800 and big["l2_hit_rate"] < 0.5
    none, why = bench.pick_pmc_record(7, 7, (1920, 1080))
    assert none is None and "no PMC record at this launch size" in why
    none, why = bench.pick_pmc_record(20, 20, (3840, 2160))
    assert none is None


def test_switches_refuse_a_null_handle_without_touching_a_device():
    """The run-time forms of the reference's compile-time switches (ABI 9 and before): a NULL handle is TWK_ERROR_INVALID_VALUE
    with a message that names the call, before any HIP call — checkable without a GPU."""
    from tweeker_raytracer_amd import _lib
    for name in ("twk_set_next_event_estimation", "twk_set_debug_exceptions", "twk_set_time_view", "twk_enable_aov", "twk_set_shader_variant"):
        rc = getattr(_lib.lib, name)(None, 1)
        assert rc == _lib.TWK_ERROR_INVALID_VALUE, name
        assert name in _lib.lib.twk_last_error().decode(), name
