"""orc_skybox against a cube map whose texels hold their own direction (tests/skybox_direction_ref.py): each pixel must
return the lookup direction skybox.wgsl prescribes, within the bilinear error of that map.  Independent of sample_cube; the
kernel side is tests/test_skybox_direction_gpu.py."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import skybox_direction_ref as S

N = 64
W, H = 97, 61          # odd: the centre column / row looks exactly along the view axis

# looking along each axis (the centre pixel's lookup vector is a face centre) and at face corners / edges
CAMERAS = {
    "+x": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0, 0, 1)),
    "-x": ((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0, 0, 1)),
    "+y": ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0, 0, 1)),
    "-y": ((0.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0, 0, 1)),
    "+z": ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0, 1, 0)),
    "-z": ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0, 1, 0)),
    "corner_ppp": ((1.0, 2.0, 3.0), (2.0, 3.0, 4.0), (0, 0, 1)),
    "corner_mpm": ((5.0, -1.0, 2.0), (4.0, 0.0, 1.0), (0, 0, 1)),
    "edge_xy": ((0.0, 0.0, 0.0), (1.0, -1.0, 0.0), (0, 0, 1)),
    "oblique": ((30.0, -7.0, 2.0), (31.0, -6.5, 2.8), (0, 0, 1)),
}


def check(out, cam, equi):
    dirs = S.lookup_dirs(cam, W, H, equi)
    err = np.linalg.norm(np.asarray(out, np.float64)[..., :3] - dirs, axis=-1)
    tol = S.tolerance(dirs, N)
    bad = err > tol
    assert not bad.any(), f"{bad.sum()} pixels off, worst {err.max():.3e} (tol there {tol.flat[err.argmax()]:.1e})"
    assert np.all(np.asarray(out)[..., 3] == 1.0)


def test_direction_cube_is_its_own_lookup():
    """The fixture: a lookup exactly at a texel centre returns that texel's direction."""
    faces = S.direction_cube(4)
    assert np.allclose(np.linalg.norm(faces[..., :3], axis=-1), 1.0, atol=1e-6)
    assert np.allclose(faces[0, 1, 2, :3] @ [1, 0, 0], faces[0, 1, 2, 0])
    assert faces[0, ..., 0].min() > 0 and faces[1, ..., 0].max() < 0 and faces[2, ..., 1].min() > 0
    assert faces[3, ..., 1].max() < 0 and faces[4, ..., 2].min() > 0 and faces[5, ..., 2].max() < 0


@pytest.mark.parametrize("equi", [0, 1])
@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_oracle_skybox_returns_the_view_direction(name, equi):
    pos, tgt, up = CAMERAS[name]
    cam = orc.Camera(W, H, pos, tgt, list(up))
    check(orc.skybox_render(cam, S.direction_cube(N), W, H, equi), cam, equi)
