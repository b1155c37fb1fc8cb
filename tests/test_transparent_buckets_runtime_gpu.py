"""The bucket route of the Transparent queue through the C++ host mirror: tests/test_transparent_runtime_gpu.py's `.renderer` text and scene with
sailor_rt_set_transparent_mode(1).  `Main` equals mode 0 and the Python route (SurfacePass.transparent, either mode) bit for bit, the depth attachment is
untouched, the overflow is the same in both modes at budgets below the scene's depth, a wrong mode is refused and changes nothing, every pass-level refusal
holds in mode 1, and a frame without transparent batches is the same in either mode."""
import numpy as np
import pytest
import torch

from sailor_amd.forward_plus import ForwardPlus, PreparedLights, SurfacePass
from test_gltf_runtime_gpu import MIXED
from test_masked_runtime_gpu import frame_launches, surface_launches
from test_transparent_runtime_gpu import ADDITIVE, ALPHA, MULTIPLY, NONE, UNSUPPORTED, TransparentScene, renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(ctx):
    return TransparentScene(ctx)


def runtime_frame(scene, mode, layers):
    """one frame of the runtime under the mode -> (status, the launches' names, Main, the depth attachment, the overflow)"""
    main, depth = scene.sky.clone(), scene.depth.clone()
    rt = scene.runtime_from(renderer(), main, depth)
    try:
        if mode is not None:
            rt.set_transparent_mode(mode)
        if layers != 4:
            rt.set_transparent_layers(layers)
        status, names = frame_launches(rt)
        torch.cuda.synchronize()
        return status, names, main.cpu().numpy(), depth.cpu().numpy(), rt.transparent_overflow()
    finally:
        rt.close()


def python_buckets(ctx, scene, layers):
    """TransparentScene.python_route with mode="buckets" -> (Main, the counters)"""
    frame, n = scene.f.cam.frame, len(scene.f.lights)
    fp = ForwardPlus(ctx, scene.W, scene.H, n, prepared=PreparedLights(ctx, scene.lights, n))
    fp.cull(frame, scene.lights, n, scene.lin)
    main = scene.sky.clone()
    sp = SurfacePass(ctx, scene.W, scene.H)
    sp.begin(scene.depth)
    scene.draw(sp, 1, gltf=True, cutout=False, cull_back=True)
    surface, _, _, _, emissive = sp.resolve_gltf(frame, scene.instances, scene.materials, scene.textures, scene.num_textures)
    sp.composite_gltf(fp.shade(frame, surface, scene.lights, n), emissive, main)
    draws = [scene.draw_args(0, True, False, False, "additive"), scene.draw_args(2, False, True, True, "alpha")]
    counts = sp.transparent(frame, draws, scene.instances, scene.materials, scene.textures, scene.num_textures, scene.depth,
                            lambda surface, ao: fp.shade(frame, surface, scene.lights, n), main, layers=layers, mode="buckets").cpu().numpy()
    ctx.synchronize()
    return main.cpu().numpy(), counts


@pytest.mark.parametrize("layers", [4, 1])
def test_main_equals_mode_0_and_the_python_route_and_the_overflow_is_the_same(ctx, scene, layers):
    want, counts = scene.python_route(ctx, layers)                  # the peel, through Python
    assert counts[0] > 1000 and counts[layers] > 0, counts         # the boxes stack deeper than either budget: both frames overflow
    by_buckets, bucket_counts = python_buckets(ctx, scene, layers)
    np.testing.assert_array_equal(by_buckets.view(np.uint32), want.view(np.uint32))
    assert bucket_counts.tolist() == counts.tolist()
    status0, names0, main0, depth0, overflow0 = runtime_frame(scene, None, layers)
    status1, names1, main1, depth1, overflow1 = runtime_frame(scene, 1, layers)
    assert status0 == 0 and status1 == 0, (status0, status1)
    np.testing.assert_array_equal(main1.view(np.uint32), main0.view(np.uint32))
    np.testing.assert_array_equal(main1.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(depth1.view(np.uint32), scene.depth.cpu().numpy().view(np.uint32))   # the attachment is read only
    assert overflow1 == overflow0 == int(counts[layers])
    # the pass by name: the draws once, a read-out a layer and one for the sentinel
    opaque = ["k_surface_begin", "k_surface_visibility_gltf", "k_surface_resolve_gltf", "k_surface_composite_gltf"]
    once = ["k_surface_begin", "k_surface_bucket", "k_surface_bucket_gltf"]
    per_layer = ["k_surface_bucket_layer", "k_surface_resolve_gltf", "k_surface_blend"]
    assert surface_launches(names1, opaque + once + per_layer * layers + per_layer[:1]), names1
    assert not any("bucket" in n for n in names0) and any(n == "k_surface_peel" for n in names0), names0


def test_a_wrong_mode_is_refused_and_changes_nothing(ctx, scene):
    rt = scene.runtime_from(renderer(), scene.sky.clone(), scene.depth.clone())
    try:
        for bad in (2, -1, 64, 2 ** 31 - 1):
            assert rt.rt.sailor_rt_set_transparent_mode(rt.h, bad) == -1
            with pytest.raises(Exception):
                rt.set_transparent_mode(bad)
        assert rt.rt.sailor_rt_set_transparent_mode(None, 1) == -1
        status, names = frame_launches(rt)                          # still the default: the peel
        assert status == 0 and any(n == "k_surface_peel" for n in names) and not any("bucket" in n for n in names), names
        rt.set_transparent_mode(1)
        assert rt.rt.sailor_rt_set_transparent_mode(rt.h, 7) == -1   # ... and mode 1 stays mode 1
        status, names = frame_launches(rt)
        assert status == 0 and any(n == "k_surface_bucket_layer" for n in names) and not any("peel" in n for n in names), names
        rt.set_transparent_mode(0)
        status, names = frame_launches(rt)
        assert status == 0 and any(n == "k_surface_peel_commit" for n in names) and not any("bucket" in n for n in names), names
    finally:
        rt.close()


def test_every_pass_level_refusal_holds_in_mode_1(ctx, scene):
    def status_of(text=None, split=False, **how):
        main, depth = scene.sky.clone(), scene.depth.clone()
        rt = scene.runtime_from(text or renderer(), main, depth, **how)
        try:
            rt.set_transparent_mode(1)
            if split:
                rt.set_frame_split(0, 2)
            status, names = frame_launches(rt)
            assert status == 0 or not any("bucket" in n for n in names), names     # nothing of a refused pass is launched
            torch.cuda.synchronize()
            return status, main.cpu().numpy()
        finally:
            rt.close()
    # z-write on and off in one pass
    assert status_of(z_write=[0, 1, 1])[0] == UNSUPPORTED
    assert status_of(z_write=[1, 1, 0])[0] == UNSUPPORTED
    # a Multiply batch: Main is the opaque pass's
    status, main = status_of(blend=[MULTIPLY, NONE, ALPHA])
    assert status == UNSUPPORTED
    np.testing.assert_array_equal(main.view(np.uint32), scene.python_route(ctx, 4, transparent=False)[0].view(np.uint32))
    # an indirect transparent pass, a split frame
    assert status_of(renderer(culling=True))[0] == UNSUPPORTED
    assert status_of(split=True)[0] == UNSUPPORTED
    assert status_of()[0] == 0 and [ADDITIVE, NONE, ALPHA] == scene.blend   # (the scene as it is passes)


def test_a_frame_without_transparent_batches_is_the_same_in_either_mode(ctx, scene):
    """tests/test_transparent_runtime_gpu.py's frame of z-writing batches through build_graph's one RenderScene node, under mode 0 and mode 1"""
    want, want_depth, _, _ = scene.through_the_c_abi(ctx, MIXED)
    for mode in (0, 1):
        rt = scene.runtime(scene.shaders)
        try:
            rt.set_transparent_mode(mode)
            rt.set_scene_blend([NONE] * 3, [1] * 3)
            main, depth = scene.sky.clone(), scene.raw.clone()
            rt.set_scene_targets(main, depth)
            status, names = frame_launches(rt)
            assert status == 0, status
            assert surface_launches(names, ["k_surface_begin", "k_surface_visibility", "k_surface_visibility_gltf", "k_surface_visibility_gltf", "k_surface_resolve_gltf",
                                            "k_surface_composite_gltf", "k_surface_store_depth"]), names
            torch.cuda.synchronize()
            np.testing.assert_array_equal(main.cpu().numpy().view(np.uint32), want.view(np.uint32))
            np.testing.assert_array_equal(depth.cpu().numpy().view(np.uint32), want_depth.view(np.uint32))
            assert rt.transparent_overflow() == 0
        finally:
            rt.close()
