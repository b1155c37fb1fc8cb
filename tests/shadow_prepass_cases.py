"""The scene of the ShadowPrepass runtime tests: a ground in four strips, a few boxes and one directional light, over a camera whose far plane is 1 000 units, so
that the four cascades end 50, 100, 333 and 500 units in front of it.

The light looks straight down.  Its cascades are then slabs along the camera's view direction that only meet at their boundaries, and every caster of SCENE sits
inside ONE slab: no caster is shared by two cascades.  That matters for the frames after the first.  The reference removes a caster from a cascade only while an
earlier cascade of the same type is re-rendered in the same frame (ECS/LightingECS.cpp:310-327); in a frame where nothing changed the earlier cascade is not
re-rendered, the later one keeps the shared caster, its list differs from its snapshot and it is drawn again -- the lists settle one cascade per frame
(tests/test_shadow_prepass_cpu.py walks through it).  With no shared caster the second unchanged frame records nothing, which is what the change-tracking test
needs; SHARED adds the one box that straddles the boundary of cascades 1 and 2, for the dependency pass and for the settling.  NumPy only; the overlap sets of
the layout are checked on the CPU by tests/test_shadow_prepass_cpu.py (oracle.csm_caster_masks)."""
import numpy as np

import surface_cases as cases
from sailor_amd import host, synth

f32 = np.float32
W, H = 128, 96
Z_FAR = 1000.0
PAD_VERTICES, PAD_INDICES, PAD_INSTANCES = 4, 3, 2
LIGHT_ROTATION = f32([np.sin(np.radians(-45.0)), 0.0, 0.0, np.cos(np.radians(-45.0))])   # -90 degrees about +X: forward (0, 0, -1) becomes (0, -1, 0)
LIGHT_POSITION = f32([0.0, 1000.0, 0.0])   # above the scene: the casters' light-clip z lies in (0, 1] (below it every fragment has z < 0 and none exists)
GROUND_Y = 60.0
# per cascade slab: the ground strip (z from, z to, half width) and the boxes (count, centre z range, centre x half range, scale range)
STRIPS = [(-4.0, -46.0, 30.0), (-54.0, -96.0, 100.0), (-106.0, -328.0, 300.0), (-340.0, -495.0, 300.0)]
BOXES = [(2, (-35.0, -15.0), 15.0, (2.0, 3.0)), (3, (-85.0, -65.0), 50.0, (3.0, 5.0)), (5, (-300.0, -130.0), 150.0, (8.0, 14.0)), (4, (-470.0, -375.0), 200.0, (10.0, 15.0))]
SHARED_BOX = ((20.0, 75.0, -100.0), 6.0)   # centre and scale: across the boundary of cascades 1 and 2


def camera(position=(0.0, 150.0, 0.0)):
    cam = synth.make_camera(W, H, z_far=Z_FAR)
    cam.world = host.transform_matrix([*position, 1.0], [0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0])
    cam.frame = host.fill_frame_data(cam.world, cam.fov, cam.z_near, cam.z_far, cam.width, cam.height)
    return cam


def light_view():
    return host.mat4_inverse(host.transform_matrix([*LIGHT_POSITION, 0.0], LIGHT_ROTATION, [1.0, 1.0, 1.0, 1.0]))


def lights_matrices(cam):
    """host cascade matrices x light matrix (sailor_host_csm_matrices): float32 [4, 16]"""
    return host.csm_matrices(light_view(), cam.world, cam.aspect, cam.fov, cam.z_near, cam.z_far)


def cascade_planes(cam):
    lm = lights_matrices(cam)
    return np.stack([host.extract_frustum_planes_matrix(lm[k])[0] for k in range(4)])


class Layout:
    """the scene as host arrays: a pool of two meshes behind padding (a cube, a unit quad in the xz plane facing up), the instances behind two unused ones, two
    batches (boxes, strips), materials and textures for RenderScene, and per instance its world box"""

    def __init__(self, shared: bool):
        rng = np.random.default_rng(77)
        p, tris = synth.unit_cube_mesh()
        cube = np.zeros((8, 18), f32)
        cube[:, 2:5] = p; cube[:, 0:2] = p[:, 0:2] * 0.5 + 0.5; cube[:, 5:8] = p / np.sqrt(3); cube[:, 8:11] = (1, 0, 0); cube[:, 11:14] = (0, 1, 0); cube[:, 14:18] = 1
        up = dict(normal=(0, 1, 0), tangent=(1, 0, 0), bitangent=(0, 0, -1))
        quad = np.stack([cases.vertex((-1, 0, 1), (0, 0), **up), cases.vertex((1, 0, 1), (8, 0), **up), cases.vertex((1, 0, -1), (8, 8), **up), cases.vertex((-1, 0, -1), (0, 8), **up)])
        self.vertices = np.concatenate([np.zeros((PAD_VERTICES, 18), f32), cube, quad])
        self.indices = np.concatenate([np.zeros(PAD_INDICES, np.uint32), tris.reshape(-1), np.uint32([0, 1, 2, 0, 2, 3])]).astype(np.uint32)
        models = [cases.IDENTITY] * PAD_INSTANCES
        self.slab_of = [-1] * PAD_INSTANCES
        for slab, (count, (z0, z1), half_x, (s0, s1)) in enumerate(BOXES):
            for _ in range(count):
                q = rng.normal(size=4)
                models.append(host.transform_matrix([rng.uniform(-half_x, half_x), rng.uniform(80.0, 110.0), rng.uniform(z0, z1), 1.0], q / np.linalg.norm(q),
                                                    [*rng.uniform(s0, s1, 3), 1.0]))
                self.slab_of.append(slab)
        if shared:
            (x, y, z), s = SHARED_BOX
            models.append(host.transform_matrix([x, y, z, 1.0], [0.0, 0.0, 0.0, 1.0], [s, s, s, 1.0]))
            self.slab_of.append(-2)
        self.num_boxes = len(models) - PAD_INSTANCES
        for slab, (za, zb, half_x) in enumerate(STRIPS):
            models.append(host.transform_matrix([0.0, GROUND_Y, 0.5 * (za + zb), 1.0], [0.0, 0.0, 0.0, 1.0], [half_x, 1.0, 0.5 * abs(za - zb), 1.0]))
            self.slab_of.append(slab)
        self.instances = cases.instances(models, [k % 2 for k in range(len(models))])
        self.num_instances = len(models)
        self.materials = np.concatenate([cases.material(albedo=(0.9, 0.8, 0.7, 1), metallic=0.3, roughness=0.6, samplers=(0, 2, 1, 2)),
                                         cases.material(albedo=(0.4, 0.6, 0.9, 1), metallic=0.8, roughness=0.3, samplers=(2, 0, 1, 0))])
        self.textures, self.srgb = [cases.distinct_texture(16, 16, 2), cases.FLAT_NORMAL, cases.distinct_texture(4, 4, 5)], [True, False, False]
        # indexCount, instanceCount, firstIndex, vertexOffset, firstInstance
        self.batches = np.uint32([[36, self.num_boxes, PAD_INDICES, PAD_VERTICES, PAD_INSTANCES],
                                  [6, len(STRIPS), PAD_INDICES + 36, PAD_VERTICES + 8, PAD_INSTANCES + self.num_boxes]])
        self.batch_ranges = [(int(b[4]), int(b[1])) for b in self.batches]
        # world boxes: the mesh's vertices through the model matrix (float64, rounded outwards); the two unused records get an empty box far away
        self.world_aabb = np.zeros((self.num_instances, 6), f32)
        self.world_aabb[:PAD_INSTANCES] = (1e6, 1e6, 1e6, 1e6, 1e6, 1e6)
        for b in self.batches:
            positions = self.vertices[int(b[3]):, 2:5][np.unique(self.indices[int(b[2]): int(b[2]) + int(b[0])])].astype(np.float64)
            for i in range(int(b[4]), int(b[4]) + int(b[1])):
                m = self.instances["model"][i].astype(np.float64).reshape(4, 4).T
                world = positions @ m[:3, :3].T + m[:3, 3]
                self.world_aabb[i, :3] = np.nextafter(world.min(0).astype(f32), f32(-np.inf))
                self.world_aabb[i, 3:] = np.nextafter(world.max(0).astype(f32), f32(np.inf))
        self.last_changed_frames = np.zeros(self.num_instances, np.uint64)

    def batch_of(self, instance: int) -> int:
        return next(j for j, (first, count) in enumerate(self.batch_ranges) if first <= instance < first + count)


def layout(shared: bool = False) -> Layout:
    return Layout(shared)
