"""Cases for row E4 as the reference runs it (RHISceneView::TraceScene through TOctree over integer-truncated world boxes), shared by
tests/test_trace_scene_cpu.py (the per-entity rule of include/sailor_hip.h against oracle.trace_scene_octree_boxes, no device) and
tests/test_trace_scene_gpu.py (the HIP entry points against both).  The rule, per entity: truncate GetCenter() / GetExtents() towards zero, insert iff the
root strictly contains the integer box, visible iff inserted, the root's own box passes and Frustum::OverlapsAABB passes on (float)p -+ (float)e; a
centre or extent component that is NaN, +-Inf or of magnitude >= 2^31 makes the entity neither inserted nor visible."""
import numpy as np

from oracle import oracle
from sailor_amd import _lib, synth

ROOT = _lib.OCTREE_ROOT_SIZE   # SAILOR_OCTREE_ROOT_SIZE; test_trace_scene_cpu.py holds it equal to the oracle's


def bits(words: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def words(b: np.ndarray) -> np.ndarray:
    n = len(b)
    padded = np.zeros(((n + 63) // 64) * 64, bool)
    padded[:n] = b
    return np.packbits(padded, bitorder="little").view(np.uint64)


def overlaps(planes, mn, mx) -> np.ndarray:
    """Frustum::OverlapsAABB (Math/Bounds.cpp:245-260) in float32, the oracle's order of operations"""
    pl = np.asarray(planes, np.float32).reshape(6, 4)
    out = np.ones(len(mn), bool)
    with np.errstate(all="ignore"):
        for i in range(6):
            d = ((np.maximum(mn[:, 0] * pl[i, 0], mx[:, 0] * pl[i, 0]) + np.maximum(mn[:, 1] * pl[i, 1], mx[:, 1] * pl[i, 1])) +
                 np.maximum(mn[:, 2] * pl[i, 2], mx[:, 2] * pl[i, 2])) + pl[i, 3]
            out &= d > 0
    return out


def trace_rule(aabb: np.ndarray, planes, root_size: int = ROOT):
    """-> (visible, inserted, defined), bool [n] each"""
    aabb = np.ascontiguousarray(aabb, np.float32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        c = (aabb[:, :3] + aabb[:, 3:]) * np.float32(0.5)
        e = (aabb[:, 3:] - aabb[:, :3]) * np.float32(0.5)
        ok = (np.abs(c) < np.float32(2.0 ** 31)) & (np.abs(e) < np.float32(2.0 ** 31))
    defined = ok.all(axis=1)
    p = np.trunc(np.where(ok, c, 0)).astype(np.int64)
    x = np.trunc(np.where(ok, e, 0)).astype(np.int64)
    h = root_size // 2
    inserted = defined & ((-h < p - x) & (h > p + x)).all(axis=1)
    pf, xf = p.astype(np.int32).astype(np.float32), x.astype(np.int32).astype(np.float32)
    hf = np.float32(root_size) * np.float32(0.5)
    root_visible = bool(overlaps(planes, np.full((1, 3), -hf, np.float32), np.full((1, 3), hf, np.float32))[0])
    visible = inserted & root_visible & overlaps(planes, pf - xf, pf + xf)
    return visible, inserted, defined


def one_plane(normal, w) -> np.ndarray:
    """a frustum whose only active plane is (normal, w): the other five have a zero normal and w = 1 (they always pass a finite box)"""
    pl = np.zeros((6, 4), np.float32)
    pl[:, 3] = 1.0
    pl[0, :3] = normal
    pl[0, 3] = w
    return pl.reshape(24)


def box(center, extent) -> list:
    c, e = np.asarray(center, np.float32), np.asarray(extent, np.float32)
    return [*(c - e), *(c + e)]


def camera_planes(width: int = 3840, height: int = 2160) -> np.ndarray:
    from sailor_amd import host
    cam = synth.make_camera(width, height)
    planes, _ = host.extract_frustum_planes(cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)
    return np.asarray(planes, np.float32).reshape(24)


def truncation_case(seed: int = 7):
    """(world boxes [n, 6], four frusta [4, 24], root size): boxes around the thresholds of three one-plane frusta and the 4K camera -- negative
    fractional centres, extents below one, finite inverted boxes (with and without a negative truncated extent), and boxes the float and the
    integer test disagree on in both directions"""
    rng = np.random.default_rng(seed)
    planes = np.stack([one_plane((1, 0, 0), -10.5),      # max x > 10.5
                       one_plane((1, 0, 0), 0.5),        # max x > -0.5
                       one_plane((-1, 0, 0), 0.5),       # min x < 0.5
                       camera_planes()])
    hand = [
        [10.0, -0.5, -0.5, 10.6, 0.5, 0.5],   # float max 10.6 passes plane 0; truncated: centre 10, extent 0 -> 10 does not
        [-2.9, -0.5, -0.5, -0.9, 0.5, 0.5],   # centre -1.9 -> -1, extent 1: integer max 0 passes plane 1, float max -0.9 does not
        [-1.2, -1.2, -1.2, -0.2, -0.2, -0.2], # centre -0.7 truncates to 0
        [0.2, 0.2, 0.2, 1.2, 1.2, 1.2],       # centre 0.7 truncates to 0
        [5.1, 5.1, 5.1, 5.9, 5.9, 5.9],       # extents below one: a point box at 5
        [-5.9, -5.9, -5.9, -5.1, -5.1, -5.1], # ... at -5
        [12.0, 3.0, 3.0, 9.0, 1.0, 1.0],      # finite inverted (min > max): extent -1.5 -> -1
        [0.6, 0.0, 0.0, -0.6, 0.0, 0.0],      # inverted around 0
        [-0.4, -0.4, -0.4, 0.4, 0.4, 0.4],    # the whole box truncates to the origin
        [10.9, 0.0, 0.0, 10.9, 0.0, 0.0],     # a point at 10.9 -> 10
        [2.0, 2.0, 2.0, 0.0, 0.0, 0.0],       # inverted, centre 1, extent -1: the walk can hide it behind a node that fails "min x < 0.5"
    ]
    c = rng.uniform(-14.0, 14.0, (4000, 3)).astype(np.float32)
    e = rng.uniform(-0.5, 3.0, (4000, 3)).astype(np.float32)
    c[:1000] = np.round(c[:1000] * 2) / 2   # half-integer centres
    e[1000:2000] = rng.uniform(0.0, 1.0, (1000, 3)).astype(np.float32)
    e[3000:] = rng.uniform(-3.0, -1.0, (1000, 3)).astype(np.float32)   # inverted by more than two units: negative truncated extents
    rnd = np.concatenate([c - e, c + e], axis=1)
    world = synth.make_entities(2000)
    _, cam_boxes, _ = oracle.ecs_sweep(world.transforms, world.parent, world.local_aabb, planes[3])
    return np.ascontiguousarray(np.concatenate([np.asarray(hand, np.float32), rnd, cam_boxes]).astype(np.float32)), planes, ROOT


def large_case(seed: int = 11):
    """centres above 2^24 under a root of 2^30: the rebuilt box (float)p -+ (float)e rounds"""
    rng = np.random.default_rng(seed)
    two25 = np.float32(2.0 ** 25)
    planes = np.stack([one_plane((1, 0, 0), -(two25 + 8)),              # max x > 2^25 + 8
                       one_plane((-1, 0, 0), two25 + 8),                # min x < 2^25 + 8
                       one_plane((0.6, 0.8, 0.0), -(two25 + 64)),
                       one_plane((0, 0, 1), -np.float32(2.0 ** 24 + 3))])
    c = np.empty((6000, 3), np.float32)
    c[:, 0] = two25 + rng.integers(-64, 64, 6000).astype(np.float32) * 2
    c[:, 1] = two25 + rng.integers(-64, 64, 6000).astype(np.float32) * 4
    c[:, 2] = np.float32(2.0 ** 24) + rng.integers(-16, 16, 6000).astype(np.float32)
    e = rng.integers(0, 12, (6000, 3)).astype(np.float32) + rng.choice(np.float32([0.0, 0.5, 0.75]), (6000, 3))
    aabb = np.concatenate([c - e, c + e], axis=1).astype(np.float32)
    return np.ascontiguousarray(aabb), planes, 1 << 30


def root_faces_case(root_size: int = 64):
    """integer faces exactly on +-h and one unit inside, on every axis, both signs"""
    h = root_size // 2
    boxes = []
    for axis in range(3):
        for p, x in ((h - 1, 1), (h - 2, 1), (-(h - 1), 1), (-(h - 2), 1), (0, h), (0, h - 1), (h - 4, 3), (h - 5, 3), (-(h - 4), 3),
                     (-(h - 5), 3), (h, 0), (h - 1, 0), (-h, 0), (-(h - 1), 0)):
            cc, ee = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            cc[axis], ee[axis] = float(p), float(x)
            boxes.append(box(cc, ee))
            ee2 = list(ee)
            ee2[axis] = x + 0.75   # fractional extent truncates back to x
            boxes.append(box(cc, ee2))
    return np.ascontiguousarray(np.asarray(boxes, np.float32)), root_size


UNDEFINED = [
    [np.nan, 0.0, 0.0, 1.0, 1.0, 1.0],
    [0.0, 0.0, 0.0, 1.0, np.nan, 1.0],
    [-np.inf, 0.0, 0.0, 1.0, 1.0, 1.0],
    [0.0, 0.0, 0.0, 1.0, 1.0, np.inf],
    [-np.inf, -np.inf, -np.inf, np.inf, np.inf, np.inf],
    [3e9, 0.0, 0.0, 3e9, 1.0, 1.0],         # centre 3e9
    [-3e9, 0.0, 0.0, -3e9, 1.0, 1.0],       # centre -3e9
    [-3e9, -1.0, -1.0, 3e9, 1.0, 1.0],      # extent 3e9
    [3e9, -1.0, -1.0, -3e9, 1.0, 1.0],      # extent -3e9 (inverted)
    [2147483648.0, 0.0, 0.0, 2147483648.0, 0.0, 0.0],  # exactly 2^31
]


def with_undefined(aabb: np.ndarray, every: int = 37) -> np.ndarray:
    """aabb with the UNDEFINED boxes spread over it (rows 5, 5 + every, ...)"""
    out = np.array(aabb, np.float32, copy=True)
    for k, b in enumerate(UNDEFINED):
        out[5 + k * every] = b
    return out


def oracle_comparable(aabb: np.ndarray) -> np.ndarray:
    """bool [n]: the boxes the oracle can be given -- defined, and p -+ e within int32 (its C integer arithmetic would overflow otherwise)"""
    aabb = np.ascontiguousarray(aabb, np.float32).reshape(-1, 6)
    _, _, defined = trace_rule(aabb, one_plane((0, 0, 0), 1.0))
    with np.errstate(all="ignore"):
        c = np.where(defined[:, None], (aabb[:, :3] + aabb[:, 3:]) * np.float32(0.5), 0)
        e = np.where(defined[:, None], (aabb[:, 3:] - aabb[:, :3]) * np.float32(0.5), 0)
    reach = np.abs(np.trunc(c).astype(np.int64)) + np.abs(np.trunc(e).astype(np.int64))
    return defined & (reach < 2 ** 31).all(axis=1)


def negative_extent(aabb: np.ndarray) -> np.ndarray:
    """bool [n]: defined boxes whose truncated extent is negative on some axis (finite, min > max by at least two units).  For those TNode::Contains
    (-h < p - e, h > p + e) is an overlap test, not a containment test: where the element rests depends on the other elements, and the walk can
    prune a node whose box fails the frustum while the element's own box passes.  The walk's visible set is then a SUBSET of the rule's (the walk
    tests the element's own box once it reaches it); its inserted bit is still the rule's (the root test alone decides it)."""
    aabb = np.ascontiguousarray(aabb, np.float32).reshape(-1, 6)
    _, _, defined = trace_rule(aabb, one_plane((0, 0, 0), 1.0))
    with np.errstate(all="ignore"):
        e = np.where(defined[:, None], (aabb[:, 3:] - aabb[:, :3]) * np.float32(0.5), 0)
    return defined & (np.trunc(e) < 0).any(axis=1)


def walk_exact(aabb: np.ndarray) -> np.ndarray:
    """bool [n]: the boxes on which the rule's visible bit is the octree walk's, whatever the other elements -- oracle_comparable, extents >= 0"""
    return oracle_comparable(aabb) & ~negative_extent(aabb)


def check_against_the_walk(vis: np.ndarray, ins: np.ndarray, ref_vis: np.ndarray, ref_ins: np.ndarray, aabb: np.ndarray) -> int:
    """vis / ins (bool [n], the rule's or the device's) against the walk's (bool [n]) on the boxes the oracle can take: inserted equal, visible
    equal where walk_exact, a superset of the walk's on negative extents.  -> how many entities the walk hides there and the rule does not"""
    keep, exact = oracle_comparable(aabb), walk_exact(aabb)
    np.testing.assert_array_equal(ins[keep], ref_ins[keep])
    np.testing.assert_array_equal(vis[exact], ref_vis[exact])
    assert not (ref_vis & ~vis)[keep].any(), "the walk sees an entity the rule does not"
    return int((vis & ~ref_vis)[keep & ~exact].sum())


def oracle_safe(aabb: np.ndarray, keep: np.ndarray, root_size: int = ROOT) -> np.ndarray:
    """aabb with the boxes not in `keep` (see oracle_comparable) replaced by a finite box outside the root"""
    out = np.array(aabb, np.float32, copy=True)
    far = np.float32(root_size)
    out[~keep] = [far, far, far, far + 1, far + 1, far + 1]
    return out


def identity_entities(aabb: np.ndarray) -> synth.EntitySet:
    """one root entity per box, identity TRS: the sweep's world box is AABB::Apply of the local box through the identity"""
    n = len(aabb)
    trs = np.zeros((n, 12), np.float32)
    trs[:, 7] = 1.0        # rotation w
    trs[:, 8:11] = 1.0     # scale
    return synth.EntitySet(transforms=trs, parent=np.full(n, 0xFFFFFFFF, np.uint32), level_offsets=np.array([0, n], np.uint32),
                           local_aabb=np.ascontiguousarray(aabb, np.float32))
