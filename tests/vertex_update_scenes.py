"""What tests/test_gpu_vertex_update.py and tests/test_gpu_temporal_carry.py share: the deformations of the geometries of
tests/selective_scenes.py. A helper module, not a conftest."""
import numpy as np

import selective_scenes as S

F = np.float32


def deformed(parts, geometry, seed=0):
    """The attributes of geometry `geometry` with new positions: a seeded displacement of at most 0.08 per coordinate for the sphere
    and the box (object space, radius / half side 1), the first corner raised by 0.15 for a wall. parts: (geometries, walls) as
    tests/test_gpu_selective_update.py's fixture gives them."""
    attributes = np.array(parts[0][geometry][0], F).reshape(-1, 12).copy()
    if geometry in (S.SPHERE, S.BOX):
        attributes[:, 0:3] += np.random.default_rng(7 + 10 * geometry + seed).uniform(-0.08, 0.08, (attributes.shape[0], 3)).astype(F)
    else:
        attributes[0, 1] += F(0.15)
    return attributes


def with_geometry(parts, new):
    """parts with {geometry: attributes} replaced: what a fresh handle is given."""
    return [(new.get(k, a), i) for k, (a, i) in enumerate(parts[0])], parts[1]
