"""GPU: the report module over the render chain (eogs2_amd.report.evaluate_views, view_products, fetch_products) on a scene of
2,000 Gaussians at 64 x 48 with three viewpoints of an MSI and a PAN camera each: `evaluate_views` equals the same chain put
together by hand — render, render_resample_virtual_camera, render_pipeline, the metrics in torch float64 — on the same
background; `view_products` returns render_set's names with their shapes, two of them checked to the bit against the
hand-made chain; `fetch_products` returns what permute(1, 2, 0).cpu().numpy() returns for each."""
import types

import numpy as np
import pytest
import torch

import report_cases as RC
import reset_cases

pytestmark = pytest.mark.gpu
H, W, P = 48, 64, 2000


@pytest.fixture(scope="module")
def scene():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    return dev, reset_cases.make_model(P, dev), RC.make_viewpoints(dev, 3, H, W), RC.make_pipe()


def by_hand(cam, model, pipe, bg):
    """train_pan.py:889-914 with this package's pieces."""
    from eogs2_amd.render import render
    from eogs2_amd.resample import render_resample_virtual_camera

    with torch.no_grad():
        bg[3] = cam.altitude_bounds[0]
        bg[4] = 0.0
        pkg = render(cam, model, pipe, bg)["render"]
        uva = torch.stack(cam.UV_grid + (pkg[3],), dim=-1)
        sun, cam2sun = cam.get_sun_camera()
        sun_rgb, sun_alt, _, sunpov = render_resample_virtual_camera(sun, cam2sun, uva, model, pipe, bg, return_extra=True)
        renderings = cam.render_pipeline(raw_render=pkg[:3], sun_altitude_diff=pkg[3] - sun_alt)
    return pkg, uva, sun_rgb, renderings


def metrics64(image, gt):
    """train_pan.py:917,942-943 in torch float64, the per-view values rounded to fp32 as the kernel rounds them."""
    d = image.double() - gt.clamp(0.0, 1.0).double()
    l1 = d.abs().mean()
    psnr = (20 * torch.log10(1.0 / torch.sqrt((d * d).view(d.shape[0], -1).mean(1)))).mean()
    return float(l1.float()), float(psnr.float())


def test_evaluate_views_equals_the_chain_by_hand(scene):
    from eogs2_amd.report import ReportAccumulator, evaluate_views

    dev, model, views, pipe = scene
    background = torch.tensor([0.2, 0.4, 0.6, 123.0, 0.7], device=dev)
    for load_msi, load_pan in ((True, True), (True, False), (False, True)):
        opt = types.SimpleNamespace(load_msi=load_msi, load_pan=load_pan, random_background=False)
        got = evaluate_views(views, model, pipe, opt, background.clone())
        sums = {"l1": {"pan": 0.0, "msi": 0.0}, "psnr": {"pan": 0.0, "msi": 0.0}}
        slack = {"l1": {"pan": 0.0, "msi": 0.0}, "psnr": {"pan": 0.0, "msi": 0.0}}
        order = []
        for vp in views:
            for cam in ([vp.get_msi_cameras()] if load_msi else []) + ([vp.get_pan_cameras()] if load_pan else []):
                order.append(cam.image_type)
                _, _, _, renderings = by_hand(cam, model, pipe, background.clone())
                l1, psnr = metrics64(renderings["shaded"], cam.original_image)
                # (one fp32 ulp per view: torch's float64 sums run in another order than the kernel's, so the one rounding to
                # fp32 may fall the other way)
                for m, v in (("l1", l1), ("psnr", psnr)):
                    sums[m][cam.image_type] += v
                    slack[m][cam.image_type] += float(RC.ulp32(v))
        assert order == [k for k, on in (("msi", load_msi), ("pan", load_pan)) if on] * len(views)  # per viewpoint MSI first, then PAN
        print(load_msi, load_pan, got)
        for m in ("l1", "psnr"):
            for kind in ("pan", "msi"):
                want = sums[m][kind] / len(views)  # by the number of viewpoints
                assert abs(got[m][kind] - want) <= slack[m][kind] / len(views), (m, kind, got[m][kind], want)
                assert np.isfinite(got[m][kind]) and (got[m][kind] != 0) == ((kind == "msi" and load_msi) or (kind == "pan" and load_pan))
    # a given accumulator is used as it stands (not reset): a second pass doubles the sums
    acc = ReportAccumulator(dev)
    acc.reset()
    opt = types.SimpleNamespace(load_msi=True, load_pan=True, random_background=False)
    once = evaluate_views(views, model, pipe, opt, background.clone(), accumulator=acc)
    twice = evaluate_views(views, model, pipe, opt, background.clone(), accumulator=acc)
    assert twice["l1"]["msi"] == 2 * once["l1"]["msi"] and acc.read()["views"] == [6, 6]
    # a random background: drawn on the device per camera, finite figures that differ from the fixed background's
    opt.random_background = True
    torch.manual_seed(0)
    rnd = evaluate_views(views, model, pipe, opt, background.clone())
    assert all(np.isfinite(rnd[m][k]) for m in rnd for k in rnd[m]) and rnd["l1"]["msi"] != once["l1"]["msi"]


def test_view_products_and_fetch(scene):
    from eogs2_amd.report import PRODUCT_KEYS, fetch_products, view_products
    from eogs2_amd.resample import render_resample_virtual_camera

    dev, model, views, pipe = scene
    background = torch.tensor([0.2, 0.4, 0.6, -9.0, 0.0], device=dev)
    for cam, planes in ((views[0].get_msi_cameras(), 3), (views[2].get_pan_cameras(), 1)):
        background[3] = cam.altitude_bounds[0]  # (render_set renders on the background it is given; by_hand writes this value)
        dsm = dict(scene_params=[(5e5, 4.3e6, 0.0), 350.0], resolution=10.0)
        products = view_products(cam, model, pipe, background.clone(), dsm=dsm)
        assert set(products) == set(PRODUCT_KEYS) | {"shadowmap", "shaded", "cc", "final", "dsm", "dsm_profile"}
        shapes = {"rawrender": (3, H, W), "altitude": (H, W), "accumulated_opacity": (H, W), "sunpovsampled": (3, H, W), "nadirpov": (3, H, W),
                  "nadirpovsampled": (3, H, W), "nadiraltitudesampled": (H, W), "nadir_altitude_diff": (H, W), "shadowmap": (H, W),
                  "shaded": (planes, H, W), "final": (planes, H, W), "gt": (planes, H, W)}
        for k, shape in shapes.items():
            assert tuple(products[k].shape) == shape and products[k].dtype == torch.float32 and not products[k].requires_grad, k
        assert products["dsm"].ndim == 3 and products["dsm"].shape[2] == 1 and products["dsm_profile"]["count"] == 1
        # the hand-made chain, on the same background
        pkg, uva, sun_rgb, renderings = by_hand(cam, model, pipe, background.clone())
        with torch.no_grad():
            nadir, cam2nadir = cam.get_nadir_camera()
            bg = background.clone()
            n_rgb, n_alt, _, nadirpov = render_resample_virtual_camera(nadir, cam2nadir, uva, model, pipe, bg, return_extra=True)
        bits = lambda a, b: a.shape == b.shape and a.contiguous().view(torch.int32).equal(b.contiguous().view(torch.int32))  # noqa: E731
        assert bits(products["sunpovsampled"], sun_rgb) and bits(products["nadir_altitude_diff"], pkg[3] - n_alt)
        assert bits(products["rawrender"], pkg[:3]) and bits(products["shaded"], renderings["shaded"]) and bits(products["nadirpov"], nadirpov[:3])
        assert float(products["nadir_altitude_diff"].abs().max()) > 0 and bits(products["gt"], cam.original_image[0:3])
        # file layout, one copy
        fetched = fetch_products(products)
        assert set(fetched) == set(products) and fetched["dsm_profile"] is products["dsm_profile"]
        for k, v in products.items():
            if not torch.is_tensor(v):
                continue
            want = (v.permute(1, 2, 0) if v.ndim == 3 and k != "dsm" else v).cpu().numpy()
            assert fetched[k].dtype == np.float32 and fetched[k].shape == want.shape, k
            assert fetched[k].tobytes() == np.ascontiguousarray(want).tobytes(), k  # NaN cells of the DSM included
    with pytest.raises(NotImplementedError):
        view_products(cam, model, pipe, background.clone(), random_camera=True)
    # gt handed in; no DSM asked for
    gt = torch.rand(1, H, W, device=dev)
    products = view_products(cam, model, pipe, background.clone(), gt=gt)
    assert products["gt"] is gt and "dsm" not in products
    # more than sixteen tensors: two launches, one buffer
    many = {f"t{i}": torch.rand((1 + i % 5, 3 + i, 5), device=dev) for i in range(19)}
    out = fetch_products(many)
    for k, v in many.items():
        assert np.array_equal(out[k], v.permute(1, 2, 0).cpu().numpy()), k
