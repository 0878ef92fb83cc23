"""CPU: the ctypes mirror of TwkVertexSource (tweeker_raytracer_amd/_lib.py VertexSource) against include/tweeker_hip.h itself: a C
program that includes the header prints sizeof and every field's offsetof, and both equal what ctypes lays out (the way
tests/test_cabi_layouts.py holds the older structs)."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

FIELDS = ("attributes", "positions", "positionStride", "recomputeFrames", "reserved")


def test_vertex_source_has_the_headers_layout(twk, tmp_path):
    L = twk._lib
    assert tuple(name for name, _ in L.VertexSource._fields_) == FIELDS
    header = os.path.join(ROOT, "include", "tweeker_hip.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {", '  printf("size %zu\\n", sizeof(TwkVertexSource));']
    lines += [f'  printf("{f} %zu\\n", offsetof(TwkVertexSource, {f}));' for f in FIELDS]
    lines += ['  printf("record %zu\\n", sizeof(TwkTriangleAttributes));', "  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    want = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert C.sizeof(L.VertexSource) == want["size"] == 40, (C.sizeof(L.VertexSource), want)
    assert {f: getattr(L.VertexSource, f).offset for f in FIELDS} == {f: want[f] for f in FIELDS}
    assert want["record"] == C.sizeof(L.TriangleAttributes) == 48
    # a zeroed source sets neither pointer, stride 0 (12), no recompute, reserved 0
    zero = L.VertexSource()
    assert zero.attributes is None and zero.positions is None and zero.positionStride == 0 and zero.recomputeFrames == 0 and list(zero.reserved) == [0, 0, 0]
