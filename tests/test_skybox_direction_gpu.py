"""k_skybox against the direction cube (tests/skybox_direction_ref.py): the cameras and bounds of
tests/test_skybox_direction_cpu.py, with the kernel in the oracle's place.  Nothing here calls orc_skybox."""
import numpy as np
import pytest

from oracle import gswt_oracle as orc
from tests import skybox_direction_ref as S
from tests.test_skybox_direction_cpu import CAMERAS, H, N, W, check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("equi", [0, 1])
def test_kernel_skybox_returns_the_view_direction(renderer, equi):
    import torch
    renderer.skybox_configure(S.direction_cube(N), bool(equi))
    for name in sorted(CAMERAS):
        pos, tgt, up = CAMERAS[name]
        cam = orc.Camera(W, H, pos, tgt, list(up))
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        renderer.skybox_render(cam.uniforms(), W, H, out.data_ptr())
        renderer.synchronize()
        check(out.cpu().numpy(), cam, equi)
