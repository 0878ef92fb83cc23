"""What tests/test_update_plan_host.py and tests/test_gpu_selective_update.py share: five small hand-made scenes as data. A helper
module, not a conftest.

Six geometries, always handed over in this order (a geometry no instance references gets no tree):
  0 light   2 triangles   the Cornell box's area light, the one instance that carries a light
  1 floor   2             2 .. 3: the box's floor, back wall and left wall, with the transforms they have there
  2 back    2
  3 side    2
  4 box     12            twk_mesh_box, 6 quads: 6 pairs
  5 sphere  48            twk_mesh_sphere(8, 4): a real tree with pair leaves
An instance is (geometry, transform, material); the light wall is instance 0 of every scene that has walls."""
import numpy as np

LIGHT, FLOOR, BACK, SIDE, BOX, SPHERE = range(6)
TRIANGLES = (2, 2, 2, 2, 12, 48)
WALLS = (LIGHT, FLOOR, BACK, SIDE)


def affine(scale, at):
    sx, sy, sz = (scale, scale, scale) if np.isscalar(scale) else scale
    return np.array([sx, 0, 0, at[0], 0, sy, 0, at[1], 0, 0, sz, at[2]], np.float32)


def rotated(at, angle=0.6, scale=(0.3, 0.2, 0.25)):
    """A rotation about y by `angle` after a non-uniform scale, then the translation."""
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag(scale)
    return np.concatenate([r, np.array(at, np.float64).reshape(3, 1)], axis=1).astype(np.float32).reshape(12)


SPHERE_AT = ((-0.4, 0.5, -0.25), (0.45, 0.45, 0.3), (0.0, 1.3, -0.3))
_spheres = lambda n: [(SPHERE, affine(0.35, SPHERE_AT[k]), 6 + (k % 2)) for k in range(n)]
_box = (BOX, affine(0.22, (0.45, 0.23, -0.35)), 2)
_boxes = [(BOX, affine(0.08, (-0.75 + 0.5 * (k % 4), 0.1 + 0.45 * (k // 4), -0.6 + 0.3 * (k // 4))), 2 + (k % 4)) for k in range(12)]

# name: (flatten policy, the instances after the walls, with walls?)
SCENES = {
    "flat": ((4, 2), [_box] + _spheres(1), True),        # all flattened: four direct-leaf walls, the box, the sphere
    "two-level": ((0, 0), _spheres(3), True),            # everything entered
    "mixed": ((0, 1), _spheres(3) + [_box], True),       # the spheres (three references) entered, walls and box flattened
    "single": ((4, 2), _spheres(1), False),              # one flattened instance and nothing else: its tree is the scene
    "many": ((12, 0), _boxes, True),                     # twelve flattened boxes: enough top-level entries for the 8-wide root
}


def instance_geometry(name):
    _, rest, walls = SCENES[name]
    return (list(WALLS) if walls else []) + [g for g, _, _ in rest]


def policy(name):
    return SCENES[name][0]


def first_movable(name):
    """Index of the first instance after the walls."""
    return len(WALLS) if SCENES[name][2] else 0


# What tests/test_gpu_selective_update.py reads out of twk_debug_snapshot_scene: the leading fields of LaunchParams (csrc/device_types.h),
# as (name, ctypes type name), and the sizes the arrays behind them have. tests/test_update_plan_host.py checks all of it against the
# headers with a compiled program, so that a reordered struct or a changed constant fails there and is never misread here.
SCENE_HEAD = (("nodes", "c_void_p"), ("topNodes", "c_void_p"), ("topNodes7", "c_void_p"), ("topRoot", "c_int"), ("topRoot2", "c_int"),
              ("wideQ", "c_void_p"), ("triangles", "c_void_p"), ("shadeTriangles", "c_void_p"))
NODE_BYTES, SLOT_BYTES, SHADE_RECORD_BYTES, TOP_NODES, TOP_NODES7, QUANTISED_NODE_BYTES = 64, 48, 128, 64, 32, 64

# "thousand": the light wall and 1100 flattened boxes; all boxes moved in one batch is 1102 node ranges, more than the 1024 the ranged
# tail keeps in LDS (bvh_build.hip TWK_TAIL_RANGES_LDS), so its search reads the table from global memory
THOUSAND = 1100
THOUSAND_POLICY = (12, 0)


def thousand_boxes():
    """[(geometry, transform, material)] of the 1100 boxes: a 44 x 25 grid in front of the back wall."""
    return [(BOX, affine(0.015, (-0.9 + 1.8 * (k % 44) / 43.0, 0.1 + 1.7 * (k // 44) / 24.0, -0.7 + 0.01 * (k % 7))), 2 + (k % 4)) for k in range(THOUSAND)]
