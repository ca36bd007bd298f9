"""Scenes of the roulette-ahead tests (tests/test_rr_ahead_cpu.py, tests/test_rr_ahead_gpu.py): a closed room whose ceiling is the light, cut into as many
emitter triangles as a case asks for, with two blocks and a slab that hide part of the ceiling from part of the room."""
import numpy as np

TRI = np.dtype([("p0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("mesh", "<u4"), ("prim", "<u4"), ("gid", "<u4")])
SHADE = np.dtype([("p", "<f4", 9), ("n", "<f4", 9), ("uv", "<f4", 6), ("mesh", "<u4"), ("prim", "<u4"), ("bsdf", "<u4"), ("lightFlags", "<u4")])
EM_OFF = 0xFFFFFFFF
CEILING = 5                 # mesh index of the ceiling in room()


def _grid(S, nx, nz, y):
    """The ceiling [-1, 1]^2 at height y as nx x nz quads (2 * nx * nz triangles), normals down."""
    xs, zs = np.linspace(-1, 1, nx + 1), np.linspace(-1, 1, nz + 1)
    parts = [S.quad((xs[i], y, zs[k]), (xs[i], y, zs[k + 1]), (xs[i + 1], y, zs[k + 1]), (xs[i + 1], y, zs[k]), flip=True) for i in range(nx) for k in range(nz)]
    return S.merge(parts)


def room(S, width=48, height=40, spp=8, sampler="independent", seed=0, maxDepth=8, grid=(1, 1), extra_light=False, lit=True, visible=True, background=None):
    """Meshes 0-4: floor and walls (the front wall closes the room, the camera is inside), 5: the ceiling - a light unless lit=False -, 6-8: two blocks and a slab
    under the ceiling; extra_light: 9, one more emitter triangle on the back wall."""
    d = S.SceneDescription()
    vf = lambda q: (q[0], q[3], q[1], q[2])               # (P, N, UV, F) -> add_mesh's (V, F, N, UV)
    white, red, green = S.diffuse((0.73, 0.73, 0.73)), S.diffuse((0.65, 0.05, 0.05)), S.diffuse((0.12, 0.45, 0.15))
    d.add_mesh(*vf(S.quad((-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1), flip=True)), bsdf=white)       # floor
    d.add_mesh(*vf(S.quad((-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1), flip=True)), bsdf=white)       # back
    d.add_mesh(*vf(S.quad((-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1), flip=True)), bsdf=red)         # left
    d.add_mesh(*vf(S.quad((1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1), flip=True)), bsdf=green)           # right
    d.add_mesh(*vf(S.quad((-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1), flip=True)), bsdf=white)           # front
    d.add_mesh(*vf(_grid(S, grid[0], grid[1], 1.0)), bsdf=S.diffuse((0, 0, 0)) if lit else white,
               light=S.area((1, 0.95, 0.9), 1.5, visible) if lit else None)
    d.add_mesh(*vf(S.box((-0.7, -1.0, -0.6), (-0.1, 0.1, 0.0))), bsdf=S.kazenstandard(baseColor=(0.75, 0.75, 0.75), roughness=0.5, metallic=0.0))
    d.add_mesh(*vf(S.box((0.1, -1.0, -0.2), (0.7, -0.4, 0.4))), bsdf=S.kazenstandard(baseColor=(0.9, 0.6, 0.2), roughness=0.3, metallic=1.0))
    d.add_mesh(*vf(S.box((-0.6, 0.55, -0.7), (0.5, 0.6, 0.1))), bsdf=white)                                   # slab: hides part of the ceiling
    if extra_light:
        d.add_mesh(np.array([[-0.2, 0.0, -0.99], [0.2, 0.0, -0.99], [0.0, 0.3, -0.99]], np.float32), np.array([[0, 1, 2]], np.uint32),
                   N=np.tile(np.array([[0, 0, 1]], np.float32), (3, 1)), bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 1, 1), 4.0, True))
    d.camera.update(width=width, height=height, fov=70.0, nearClip=0.01, farClip=100.0, toWorld=S.look_at((0.05, 0.1, 0.95), (0, -0.15, -1), (0, 1, 0)))
    d.sampler = {"type": sampler, "sampleCount": spp, "seed": seed}
    d.integrator["maxDepth"] = maxDepth
    d.background = background
    return d


def panel_room(S, width=48, height=40, spp=8, maxDepth=6):
    """The room with a diffuse ceiling and, instead, a light panel of lightPrimaryVisibility = false hanging in view: first hits on it are walked through (H6)."""
    d = room(S, width, height, spp, maxDepth=maxDepth, lit=False)
    q = S.quad((-0.5, 0.3, -0.6), (-0.5, 0.3, 0.4), (0.5, 0.3, 0.4), (0.5, 0.3, -0.6), flip=True)
    d.add_mesh(q[0], q[3], q[1], q[2], bsdf=S.diffuse((0, 0, 0)), light=S.area((1, 1, 1), 6.0, False))
    d.camera.update(toWorld=S.look_at((0.05, -0.2, 0.95), (0, 0.5, -1), (0, 1, 0)))
    return d


def glass_room(S, width=48, height=40, spp=8, maxDepth=8):
    """The room with a glass sphere and regularisation: eta != 1 along a path, the non-compact path state and the kernel variant of the other BSDF models."""
    d = room(S, width, height, spp, maxDepth=maxDepth, grid=(2, 2))
    P, N, UV, F = S.uv_sphere((0.35, -0.1, 0.3), 0.3, 20, 21)
    d.add_mesh(P, F, N, UV, bsdf=S.dielectric())
    d.integrator.update(regularization=True, accumulatedRoughness=0.5)
    return d


def emitter_table(kz, sc, device=-1):
    """(rows, lo, hi, count) of KZ_TABLE_EM_TRIS: the emitter triangles and the header row behind them."""
    t = sc.table(kz.abi.KZ_TABLE_EM_TRIS, device).view(TRI)
    assert len(t) >= 1
    head = t[-1]
    return t[:-1], head["p0"].copy(), head["e1"].copy(), int(head["mesh"])
