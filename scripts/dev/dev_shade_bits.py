"""sha256 of the shaded image of every shade family with the library BHGEO_LIB names -- run once per build and compare the lines (a
change under the shade kernels must not move a bit): python scripts/dev/dev_shade_bits.py
Scene shade: plain, redshift, observer, textured, polarised (rgba and qu), thermal, moving; the layered and the retarded layered
shade; the mesh and the mesh material shade.  Each at S = 1, 5 and 300 (the LDS kernel, and the serial one), the fp64 image and
the fp32 image scattered through a permutation."""
import hashlib, os, sys
import numpy as np, torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import mesh_material_cases as mmc
from blackhole_geodesic_calculator_amd import _ffi
from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame, synthetic_sky

ctx = _ffi.Context(0)
INC = np.radians(70.0)
CAM = np.array([30 * np.sin(INC), 0.0, 30 * np.cos(INC)])
DISK = (3.0, 12.0)
BETA = (0.3, -0.2, 0.1)
NU = (3.0e14, 6.0e14, 1.0e15, 1.5e15)
WEIGHTS = np.array([[1.0, 0.5, 0.1, 0.0], [0.2, 1.0, 0.4, 0.1], [0.0, 0.1, 0.6, 1.0]])
ALL = ("disk", "objects", "sky")
sky, tex, ball = synthetic_sky(256, 128), synthetic_sky(128, 32, seed=3), synthetic_sky(64, 32, seed=5)
lib = os.path.basename(os.environ.get("BHGEO_LIB", "tree"))


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:24]


def report(name, fr, stokes=False):
    if stokes:
        rgba, qu = fr.shade_stokes()
        print(name, fr.S, "qu", sha(qu))
    else:
        rgba = fr.shade()
    print(name, fr.S, "f64", sha(rgba))
    scatter = torch.as_tensor(np.random.default_rng(1).permutation(fr.P)).to(fr.dev)
    out = torch.zeros((fr.P, 4), dtype=torch.float32, device=fr.dev)
    fr.shade_f32(out, scatter=scatter)
    print(name, fr.S, "f32", sha(out), flush=True)


def disk_frame(S, spheres):
    fr = DeviceFrame(ctx, 48, 48, S, fov_x=0.9, fov_y=0.9, origin=CAM, rotation_euler=(0.0, INC, 0.0))
    fr.set_sky(sky)
    fr.set_disk(DISK[0], DISK[1], tex, disk_phase=0.4, disk_mean=0.3, disk_stddev=0.25, disk_intensity=2.0)
    if spheres:
        fr.set_objects([[6.0, 3.0, 2.5, 1.5], [2.0, 6.0, -1.0, 1.2]], [[1.0, 0.8, 0.6], [0.5, 0.5, 1.0]], [[20.0, 0.0, 20.0, 10.0]])
    return fr


print("library", lib)
for S in (1, 5, 300):
    p = _ffi.make_params(r_s=1.0, lambda_end=120.0, r_exit=40.0, disk_r_in=DISK[0], disk_r_out=DISK[1])
    fr = disk_frame(S, True)
    fr.generate_rays(p)
    fr.trace(p)
    report("plain", fr)
    fr.set_redshift(ALL, 4.0)
    report("redshift", fr)
    fr.observer = _ffi.make_observer(BETA)      # the shade's observer: the rays stay the traced ones
    report("observer", fr)
    fr.observer = None
    fr.set_redshift(None)
    fr.set_object_textures(textures=[ball], rotations=[np.eye(3)], modes=["emissive"], emission=[2.0])
    report("textured", fr)
    fr.set_object_textures()
    fr.set_polarisation((0.0, 0.35, 0.2, 0.117))
    report("polarised", fr, stokes=True)
    fr.set_polarisation(None)
    fr.set_redshift(("sky",), 4.0)
    fr.set_disk_thermal(1.2e4, NU, WEIGHTS, 1.7, 2.5, 1)
    report("thermal", fr)
    fr.set_disk_thermal(None)
    fr.set_redshift(ALL, 4.0)
    fr.set_object_motion([[0.0, 0.3, 0.1], [-0.2, 0.0, 0.0]], [[0.0, 0.0, 0.2], [0.1, 0.0, 0.0]])
    report("moving", fr)
    for name, rate in (("layers", 0.0), ("retarded", 0.05)):
        fr = disk_frame(S, False)
        fr.set_disk_layers(3, 0.5, phase_rate=rate)
        fr.generate_rays(p)
        fr.trace(p)
        report(name, fr)
    V, F = mmc.SHADE_MESH
    M = mmc.material_arrays()
    mesh = _ffi.Mesh(ctx, V, F, vertex_normals=mmc.vertex_normals())
    pm = _ffi.make_params(r_s=1.0, lambda_end=70.0, r_exit=40.0, disk_r_in=mmc.SHADE_DISK[0], disk_r_out=mmc.SHADE_DISK[1])
    for name, kw in (("mesh", dict(tri_rgb=M["tri_rgb"])), ("material", dict(material=_ffi.MeshMaterial(**M)))):
        fr = mmc.device_frame(ctx, S, fov=(0.8, 0.8))
        fr.set_mesh(mesh, chord=mmc.CHORD, **kw)
        fr.generate_rays(pm)
        fr.trace(pm)
        report(name, fr)
    mesh.close()
