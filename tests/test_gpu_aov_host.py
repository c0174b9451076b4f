"""The aov integrator end to end through the reference-shaped surface on the GPU: XML -> the `aov` plugin -> Integrator::render ->
bf_scene_set_aovs + BF_FLAG_AOV -> film.bitmap(raw=True), channel names and every cell against tests/aov_ref.py on the very
description the host flattened."""
import numpy as np
import pytest

from beifong_amd import capi
from tests import aov_ref as ar

pytestmark = pytest.mark.gpu

AOV_FILM_SCENE = """
<scene version="2.1.0">
    <integrator type="aov">
        <string name="aovs" value="dd.y:depth,nn:sh_normal,pp:position,tex:uv"/>
        <integrator type="range" name="my_image"><integrator type="pathlength"/><float name="dr" value="0.5"/><integer name="bins" value="20"/></integrator>
    </integrator>
    <sensor type="perspective">
        <float name="fov" value="90"/><float name="near_clip" value="0.1"/><float name="far_clip" value="100"/>
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, 0, 1" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="2"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="128"/></sampler>
    </sensor>
    <shape type="rectangle">
        <transform name="to_world"><rotate y="1" angle="180"/><translate x="1" z="2"/></transform>
        <emitter type="area"><spectrum name="radiance" value="3"/></emitter>
    </shape>
</scene>
"""


@pytest.fixture(scope="module")
def mitsuba():
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def test_aov_film_through_the_plugin_surface(mitsuba, hiplib):
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(AOV_FILM_SCENE)
    sensor = scene.sensors()[0]
    integ = scene.integrator()
    integ.render(scene, sensor)
    film = sensor.film()
    bmp = np.array(film.bitmap(raw=True))
    names = film.bitmap(raw=True).channel_names()
    own = ["dd.y", "nn.X", "nn.Y", "nn.Z", "pp.X", "pp.Y", "pp.Z", "tex.U", "tex.V"]
    assert names == ["X", "Y", "Z", "A", "W"] + own + [f"my_image.S{i}.Y" for i in range(20)] + ["my_image.R", "my_image.G", "my_image.B", "my_image.A"]
    assert bmp.shape == (2, 4, 38) and bmp.dtype == np.float32
    lp = integ.launch_for(sensor)
    assert lp.flags & capi.BF_FLAG_AOV and (lp.film_width, lp.film_height, lp.spp, lp.n_paths) == (4, 2, 128, 1024)
    exp, _, _ = ar.expected(scene.flat_desc(sensor), lp, ["depth", "sh_normal", "position", "uv"])
    exp.check(bmp, "aov film through the plugin surface")
    # the rectangle fills the left half of the film, 2 m away, facing the camera
    assert np.array_equal(bmp[:, :, 3], [[128, 128, 0, 0]] * 2) and np.array_equal(bmp[:, :, 37], bmp[:, :, 3])
    assert np.array_equal(bmp[:, :2, names.index("pp.Z")], np.full((2, 2), 256.0)) and not bmp[:, 2:, 5:14].any()
    assert np.array_equal(bmp[:, :2, names.index("nn.Z")], np.full((2, 2), -128.0))
    assert np.all(bmp[:, :2, 5] > 256.0)
    st, _ = integ.stats()
    assert st.kernel_variant & capi.BF_VARIANT_AOV and st.n_paths == 1024
