"""CPU: every module's refusal of tensors that are not on the GPU, word for word. The refusals are raised before any launch
by the shared checks of eogs2_amd/_host.py (`on_device`, `Ctx`, `f32c`), each in the words of the module it serves; the
literals are the messages the modules raised while each still carried a private copy of its check.

Not covered, because their checks of the device come first and need a GPU to pass: the `f32c` labels of eogs2_amd.pan
("pan_shade: <name> on <device>, expected <device>") and eogs2_amd.randomcam ("cmloss: <name> on ...")."""
import pytest
import torch

z = torch.zeros
TAIL = "on the GPU only, there is no CPU fallback"


def _flow():
    from eogs2_amd.flow import apply_flow
    apply_flow(z(1, 4, 4), z(1, 2, 4, 4))


def _dsm_eval():
    from eogs2_amd.dsm_eval import downsample2x
    downsample2x(z(4, 4))


def _dsm_raster():
    from eogs2_amd.dsm_raster import cloud_bounds
    cloud_bounds(z(3, 3, dtype=torch.float64))


def _dsm_raster_non_tensor():
    from eogs2_amd.dsm_raster import cloud_bounds
    cloud_bounds([[0.0, 0.0, 0.0]])


def _regularizers():
    from eogs2_amd.regularizers import gaussian_regularizers
    gaussian_regularizers(z(4, 1), n_init=4, weights=(1.0, 0.0, 0.0))


def _pansharp():
    from eogs2_amd.pansharp import brovey_pansharp
    brovey_pansharp(z(4, 4), z(3, 2, 2))


def _density():
    from eogs2_amd.density import add_densification_stats
    add_densification_stats(z(4, 1), z(4, 1), z(4), z(4, 3), z(4, dtype=torch.int32))


def _mesh():
    from eogs2_amd.mesh import marching_cubes
    marching_cubes(z(2, 2, 2))


def _mesh_non_tensor():
    from eogs2_amd.mesh import marching_cubes
    marching_cubes([0.0])


def _monitor():
    from eogs2_amd.monitor import TrainingMonitor
    TrainingMonitor("cuda:0").end_iteration(z(()))  # (constructing a monitor touches no device)


def _monitor_non_tensor():
    from eogs2_amd.monitor import TrainingMonitor
    TrainingMonitor("cuda:0").end_iteration(0.5)


def _tsdf():
    from eogs2_amd.tsdf import normals
    normals(z(4, 4), torch.eye(3), z(3))


def _rescaler():
    from eogs2_amd.rescaler import compute_min_vals
    compute_min_vals(z(3, 4, 4))


def _ctx():
    from eogs2_amd.knn import distCUDA2
    distCUDA2(z(5, 3))


def _f32c_losses():
    from eogs2_amd.losses import l1_loss
    l1_loss(z(3, 8, 8), z(3, 8, 8, device="meta"))


def _f32c_resample():
    from eogs2_amd.resample import resample
    resample(z(4, 8, 8), torch.eye(3), z(8, 8, 3, device="meta"))


def _f32c_shade():
    from eogs2_amd.shade import shade
    shade(z(3, 8, 8), None, z(3, 4, device="meta"), None)


CASES = [
    (_flow, RuntimeError, f"flow apply_flow: tensors live on 'cpu'; the flow warp runs {TAIL}"),
    (_dsm_eval, RuntimeError, f"dsm_eval downsample2x: tensors live on 'cpu'; the DSM evaluation runs {TAIL}"),
    (_dsm_raster, RuntimeError, f"dsm_raster cloud_bounds: tensors live on 'cpu'; the DSM raster runs {TAIL}"),
    (_dsm_raster_non_tensor, TypeError, "dsm_raster cloud_bounds: expected a tensor, not list"),
    (_regularizers, RuntimeError, f"regularizers gaussian_regularizers: tensors live on 'cpu'; the regularisers run {TAIL}"),
    (_pansharp, RuntimeError, f"pansharp brovey_pansharp: tensors live on 'cpu'; ground-truth preparation runs {TAIL}"),
    (_density, RuntimeError, f"density add_densification_stats: tensors live on 'cpu'; density control runs {TAIL}"),
    (_mesh, RuntimeError, f"mesh marching_cubes: tensors live on 'cpu'; the mesh extraction runs {TAIL}"),
    (_mesh_non_tensor, TypeError, "mesh marching_cubes: expected a tensor, not list"),
    (_monitor, RuntimeError, f"monitor end_iteration: tensors live on 'cpu'; the monitor runs {TAIL}"),
    (_monitor_non_tensor, TypeError, "monitor end_iteration: expected a tensor, got float"),
    (_tsdf, RuntimeError, f"tsdf normals: tensors live on 'cpu'; the TSDF stages run {TAIL}"),
    (_rescaler, RuntimeError, f"rescaler channel_minmax: tensors live on 'cpu'; ground-truth preparation runs {TAIL}"),
    (_ctx, RuntimeError, "rasterizer tensors live on 'cpu' but the loaded library (hip-gfx950) works on 'cuda' memory; there is no "
                         "CPU fallback"),
    (_f32c_losses, RuntimeError, "loss input on meta, expected cpu"),
    (_f32c_resample, RuntimeError, "resample input on meta, expected cpu"),
    (_f32c_shade, RuntimeError, "shade input on meta, expected cpu"),
]


@pytest.mark.parametrize("entry,kind,message", CASES, ids=[c[0].__name__.lstrip("_") for c in CASES])
def test_refusal_word_for_word(entry, kind, message):
    with pytest.raises(kind) as e:
        entry()
    assert type(e.value) is kind and str(e.value) == message
