"""GSWTRenderer.options on the GPU: what a block sets holds inside it and nowhere else.  GSWT_OPT_GRAPH is the witness: a frame
submitted under it, and no other, raises graph_stats()[0].  The grid case at 64 x 48."""
import pytest

from oracle import gswt_oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu


def test_options_hold_inside_the_block_nest_and_are_put_back(renderer):
    import torch
    pp = H.tileset()
    H.grid_case(pp).upload(renderer)
    renderer.configure(None)
    W, Hh = 64, 48
    cam, su = orc.default_camera(W, Hh).uniforms(), orc.scene_uniforms(num_lod=pp.n_lod)
    out = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def launches_of_a_frame():
        before = renderer.graph_stats()[0]
        renderer.render_wait(renderer.render_async(cam, su, W, Hh, out.data_ptr()))
        return renderer.graph_stats()[0] - before

    assert launches_of_a_frame() == 0
    with renderer.options(GRAPH=1, TIMING=0):
        assert launches_of_a_frame() == 1 and launches_of_a_frame() == 1
        with renderer.options(GRAPH=0):
            assert launches_of_a_frame() == 0
        assert launches_of_a_frame() == 1                      # the inner block put back the outer block's value, not the default
    assert launches_of_a_frame() == 0
    with pytest.raises(ZeroDivisionError):
        with renderer.options(GRAPH=1, TIMING=0):
            assert launches_of_a_frame() == 1
            1 / 0
    assert launches_of_a_frame() == 0
    with pytest.raises(KeyError):
        with renderer.options(GRAPH=1, DEPTH_PASSES=2):        # not a plain option: refused before anything is set
            pass
    assert launches_of_a_frame() == 0
    assert out.cpu().numpy()[..., 3].max() > 0.0
