"""The scene and the material the mesh-material GPU tests share: test_gpu_mesh.py's shade scene, copied --
two components placed so that the tetrahedron stands between the first lamp and the sphere -- and a material that exercises
every branch of the texel: three images of odd sizes, triangles without a slot, corner UVs on both sides of [0, 1]."""
import numpy as np

import mesh_reference as mr

SHADE_CAM = np.array([16.0, -3.0, 5.0])
SPHERE_C, TETRA_C = (-2.5, 2.0, 0.8), (-0.4, 4.6, 1.9)
SHADE_MESH = mr.join(mr.octa_sphere(SPHERE_C, 1.3, 2), mr.tetrahedron(TETRA_C, 0.8))
SHADE_LAMPS = [[4.0, 10.0, 4.0, 9.0], [12.0, -9.0, 7.0, 7.0]]
SHADE_DISK = (2.0, 7.0)
SHADE_AIM = np.array([-1.2, 2.6, 1.1])
CHORD = 0.2
EMISSION = 0.3


def camera_euler():
    look = (SHADE_AIM - SHADE_CAM) / np.linalg.norm(SHADE_AIM - SHADE_CAM)
    # (rotation_euler: the camera looks down its own -z; aim that between the hole and the mesh)
    return (float(np.arccos(-look[2])), 0.0, float(np.arctan2(-look[0], look[1])))


def vertex_normals():
    V, F = SHADE_MESH
    centres = np.where((np.arange(len(V)) < V.shape[0] - 4)[:, None], np.array(SPHERE_C), np.array(TETRA_C))
    n = V - centres
    return n / np.linalg.norm(n, axis=1)[:, None]


def material_arrays(seed=7):
    """dict(tri_rgb, tri_uv, tri_tex, textures, emission): random colours, per-corner UVs in [-1.5, 2.5], images of 7 x 5, 1 x 1 and
    16 x 16, slots drawn from {-1, 0, 1, 2}."""
    nt = len(SHADE_MESH[1])
    rng = np.random.default_rng(seed)
    return dict(tri_rgb=rng.uniform(0.2, 1.0, (nt, 3)).astype(np.float32),
                tri_uv=rng.uniform(-1.5, 2.5, (nt, 3, 2)).astype(np.float32),
                tri_tex=rng.integers(-1, 3, nt).astype(np.int32),
                textures=[rng.random((5, 7, 4)).astype(np.float32), rng.random((1, 1, 4)).astype(np.float32),
                          rng.random((16, 16, 4)).astype(np.float32)],
                emission=EMISSION)


def device_frame(ctx, S, W=32, H=32, fov=(0.5, 0.5), disk=True, **kw):
    from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky
    fr = DeviceFrame(ctx, W, H, S, fov_x=fov[0], fov_y=fov[1], origin=SHADE_CAM, rotation_euler=camera_euler(), **kw)
    fr.set_sky(synthetic_sky(128, 64))
    if disk:
        fr.set_disk(*SHADE_DISK)
    fr.set_objects([], lamps=SHADE_LAMPS)
    return fr


# ---- the library-owned frame (test_gpu_frame_mesh.py and its child process) -----------------------------------------------
FRAME_W, FRAME_H, FRAME_S, FRAME_FOV = 96, 64, 2, (0.75, 0.5)


def frame(f, devices, gather, disk=True):
    """An _ffi.Frame on the shade scene, 96 x 64 x 2, tile 16; no mesh yet."""
    from blackhole_geodesic_calculator_amd.device_frame import synthetic_sky
    from blackhole_geodesic_calculator_amd.raygen import euler_xyz_matrix, python_random_stream
    fr = f.Frame(devices, FRAME_W, FRAME_H, FRAME_S, fov_x=FRAME_FOV[0], fov_y=FRAME_FOV[1], origin=SHADE_CAM,
                 rot=euler_xyz_matrix(camera_euler()), jitter=python_random_stream(42.0, 2 * FRAME_S * FRAME_W * FRAME_H), tile=16,
                 gather=gather)
    fr.set_scene(synthetic_sky(128, 64), disk=SHADE_DISK if disk else None, lamps=SHADE_LAMPS)
    return fr


def frame_params(f, disk=True, kerr=False):
    if kerr:      # a / M = 0.9 with M = r_s / 2
        return f.make_params(r_s=1.0, lambda_end=70.0, rhs_form=f.RHS_KERR_BL, spin=0.45)
    return f.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=SHADE_DISK[0] if disk else 0.0,
                         disk_r_out=SHADE_DISK[1] if disk else 0.0)


def set_frame_mesh(f, fr, smooth=True):
    V, F = SHADE_MESH
    fr.set_mesh(V, F, vertex_normals=vertex_normals() if smooth else None, chord=CHORD, material=f.MeshMaterial(**material_arrays()))
