"""The frames of a positions-mode device source (csrc/vertex_source_device.h "FRAMES"), restated in numpy operation by operation in
float32, and once more in float64 for the accuracy bound; the meshes tests/test_vertex_frames_host.py and the stand-alone sanitizer
program share. A helper module, not a conftest.

    adjacency   per vertex the triangles that name it, ascending, each once
    s           (+0, +0, +0), then + cross(p[i1] - p[i0], p[i2] - p[i0]) per adjacent triangle in that order
    n'          s * (1 / sqrt(dot(s, s))), or the old normal without a triangle or when dot(s, s) is zero or not finite
    t*          t - n' * dot(n', t);  t' = t* * (1 / sqrt(dot(t*, t*))), or the old tangent when dot(t*, t*) is zero or not finite
    dot(a, b)   (a.x b.x + a.y b.y) + a.z b.z;  cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)"""
import numpy as np

F32 = np.float32


def adjacency(indices, num_vertices):
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    lists = [[] for _ in range(num_vertices)]
    for t, triple in enumerate(tri):
        for v in dict.fromkeys(int(i) for i in triple):  # each triangle once per vertex
            lists[v].append(t)
    return lists


def _dot(a, b, kind):
    return kind(kind(kind(a[0] * b[0]) + kind(a[1] * b[1])) + kind(a[2] * b[2]))


def _cross(a, b, kind):
    return [kind(kind(a[1] * b[2]) - kind(a[2] * b[1])), kind(kind(a[2] * b[0]) - kind(a[0] * b[2])), kind(kind(a[0] * b[1]) - kind(a[1] * b[0]))]


def frames(positions, indices, before, kind=F32):
    """The records [n, 12] after the call, every operation rounded to `kind` (float32: the definition; float64: the reference of the
    accuracy bound, whose results stay float64 in columns 3..8)."""
    p = np.asarray(positions, F32).reshape(-1, 3).astype(kind)
    tri = np.asarray(indices, np.int64).reshape(-1, 3)
    old = np.asarray(before, F32).reshape(-1, 12)
    out = old.astype(kind).copy()
    out[:, 0:3] = p
    with np.errstate(all="ignore"):
        for v, triangles in enumerate(adjacency(indices, p.shape[0])):
            s = [kind(0.0)] * 3
            for t in triangles:
                p0, p1, p2 = p[tri[t, 0]], p[tri[t, 1]], p[tri[t, 2]]
                c = _cross([kind(p1[k] - p0[k]) for k in range(3)], [kind(p2[k] - p0[k]) for k in range(3)], kind)
                s = [kind(s[k] + c[k]) for k in range(3)]
            tangent, normal = [kind(x) for x in old[v, 3:6]], [kind(x) for x in old[v, 6:9]]
            ss = _dot(s, s, kind)
            if triangles and ss > 0 and np.isfinite(ss):
                inv = kind(kind(1.0) / np.sqrt(ss))
                normal = [kind(s[k] * inv) for k in range(3)]
            d = _dot(normal, tangent, kind)
            ts = [kind(tangent[k] - kind(normal[k] * d)) for k in range(3)]
            tt = _dot(ts, ts, kind)
            if tt > 0 and np.isfinite(tt):
                inv = kind(kind(1.0) / np.sqrt(tt))
                tangent = [kind(ts[k] * inv) for k in range(3)]
            out[v, 3:6], out[v, 6:9] = tangent, normal
    return out


def positions_only(positions, before):
    """recomputeFrames 0: the records with vertex[] replaced."""
    out = np.array(before, F32).reshape(-1, 12).copy()
    out[:, 0:3] = np.asarray(positions, F32).reshape(-1, 3)
    return out


# ---- the meshes: (name, attributes [n, 12], indices) ------------------------------------------------------------------------------
def _records(positions, tangent=(1.0, 0.0, 0.0), normal=(0.0, 0.0, 1.0)):
    p = np.asarray(positions, F32).reshape(-1, 3)
    a = np.zeros((p.shape[0], 12), F32)
    a[:, 0:3], a[:, 3:6], a[:, 6:9] = p, np.asarray(tangent, F32), np.asarray(normal, F32)
    a[:, 9:11] = p[:, 0:2]
    return a


def meshes(twk):
    sphere = twk.mesh_sphere(12, 6, 1.0, np.pi)
    box = twk.mesh_box()
    out = [("sphere 12 x 6", np.array(sphere[0], F32).reshape(-1, 12), np.array(sphere[1], np.uint32).reshape(-1)),
           ("box", np.array(box[0], F32).reshape(-1, 12), np.array(box[1], np.uint32).reshape(-1)),
           ("one triangle", _records([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([0, 1, 2], np.uint32)),
           # vertex 3 is named by no index: it keeps its normal whatever the positions are
           ("an unnamed vertex", _records([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5]]), np.array([0, 1, 2], np.uint32)),
           # two triangles on vertex 0 with opposite winding over the same three points: their cross products cancel exactly
           ("a fan folded flat", _records([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 1, 0]]), np.array([0, 1, 2, 0, 4, 3], np.uint32)),
           # the tangent of every vertex is the triangle's normal: t* is exactly zero
           ("a tangent along the normal", _records([[0, 0, 0], [1, 0, 0], [0, 1, 0]], tangent=(0.0, 0.0, 1.0)), np.array([0, 1, 2], np.uint32))]
    return out
