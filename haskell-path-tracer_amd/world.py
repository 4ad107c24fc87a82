"""Scene.World -- the reference's static world as run-time data.

`main_scene()` and `initial_camera()` restate src/Scene/World.hs:8-77 value for value (they are
data, not code).  `scene16()` is the build-defined "~16 primitives" benchmark scene of
SURVEY.md 8(d): main scene + a 3x3 grid of unit spheres.
"""
import numpy as np

MATTE, GLOSSY = 0, 1          # data Brdf = Matte Float | Glossy Float  (src/Scene/Objects.hs:77-87)
GLASS = 2                     # build-defined extension (no reference semantics); parameter = index of refraction
STREAMS, INLINE = 0, 1        # data Algorithm = Streams | Inline        (src/Scene/Trace.hs:68)

# field order = src/Scene/Objects.hs (Sphere :126-131, Plane :103-108, Material :90-100, Camera :67-74)
SPHERE_DTYPE = np.dtype([("position", "<f4", 3), ("radius", "<f4"), ("color", "<f4", 3),
                         ("illuminance", "<f4"), ("brdf_tag", "<i4"), ("brdf_param", "<f4")])
PLANE_DTYPE = np.dtype([("position", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3),
                        ("illuminance", "<f4"), ("brdf_tag", "<i4"), ("brdf_param", "<f4")])
CAMERA_DTYPE = np.dtype([("position", "<f4", 3), ("rotation", "<f4", 3), ("fov", "<i8")])
# ptmi_triangle (extension: the reference has no triangle type): three vertices, counter-clockwise seen from the front, and a material
TRIANGLE_DTYPE = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3), ("color", "<f4", 3),
                           ("illuminance", "<f4"), ("brdf_tag", "<i4"), ("brdf_param", "<f4")])
assert SPHERE_DTYPE.itemsize == 40 and PLANE_DTYPE.itemsize == 48 and CAMERA_DTYPE.itemsize == 32 and TRIANGLE_DTYPE.itemsize == 60


def sphere(position, radius, color, illuminance, brdf_tag, brdf_param):
    return (tuple(position), radius, tuple(color), illuminance, brdf_tag, brdf_param)


def plane(position, direction, color, illuminance, brdf_tag, brdf_param):
    return (tuple(position), tuple(direction), tuple(color), illuminance, brdf_tag, brdf_param)


def triangle(v0, v1, v2, color, illuminance, brdf_tag, brdf_param):
    return (tuple(v0), tuple(v1), tuple(v2), tuple(color), illuminance, brdf_tag, brdf_param)


def initial_camera():
    """src/Scene/World.hs:8-12"""
    cam = np.zeros((), dtype=CAMERA_DTYPE)
    cam["position"] = (1.0, -1.6, -4.8)
    cam["rotation"] = (0.314, -0.314, 0.0)
    cam["fov"] = 90
    return cam


def camera(position, rotation, fov):
    cam = np.zeros((), dtype=CAMERA_DTYPE)
    cam["position"] = position
    cam["rotation"] = rotation
    cam["fov"] = fov
    return cam


def main_scene():
    """src/Scene/World.hs:15-77 -> (spheres, planes)"""
    spheres = np.array([
        sphere((2.0, 2.0, -14.0), 5.0, (1.0, 0.3, 0.3), 0.0, MATTE, 0.8),
        sphere((6.0, 2.0, -9.0), 1.5, (0.0, 0.4, 0.0), 0.0, MATTE, 0.9),
        sphere((4.5, 1.0, -9.0), 0.5, (0.4, 0.4, 1.0), 0.0, GLOSSY, 1.0),
        sphere((16.0, -2.05, -20.0), 0.9, (0.8, 0.8, 0.8), 6942.0, GLOSSY, 0.5),
        sphere((5.0, 10.0, 4.0), 2.0, (0.99, 0.84, 0.12), 4420.0, MATTE, 1.0),
    ], dtype=SPHERE_DTYPE)
    planes = np.array([
        plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.43, 0.95, 0.5), 0.0, MATTE, 1.5),
        plane((0.0, 15.0, 0.0), (0.0, -1.0, 0.0), (0.26, 0.68, 0.88), 0.0, GLOSSY, 0.9),
    ], dtype=PLANE_DTYPE)
    return spheres, planes


def scene16():
    """SURVEY.md 8(d) scene S16: main scene + 9 unit spheres, centres (-6+6i, 0, -6-6j)."""
    spheres, planes = main_scene()
    extra = []
    for i in range(3):
        for j in range(3):
            tag, p = (MATTE, 0.9) if (i + j) % 2 == 0 else (GLOSSY, 0.8)
            extra.append(sphere((-6.0 + 6.0 * i, 0.0, -6.0 - 6.0 * j), 1.0,
                                (0.2 + 0.3 * i, 0.5, 0.2 + 0.3 * j), 0.0, tag, p))
    spheres = np.concatenate([spheres, np.array(extra, dtype=SPHERE_DTYPE)])
    return spheres, planes


def glass_scene():
    """BASELINE.json configs[4] ("glass / refraction-heavy scene"): scene16 with the big sphere and four of the
    grid spheres turned into GLASS (ior 1.5 / 1.33).  Build-defined; the reference has no such material."""
    spheres, planes = scene16()
    spheres = spheres.copy()
    for i, ior in ((0, 1.5), (5, 1.5), (7, 1.33), (9, 1.5), (11, 1.33)):
        spheres["brdf_tag"][i] = GLASS
        spheres["brdf_param"][i] = ior
        spheres["color"][i] = (0.95, 0.95, 0.95)
    return spheres, planes


def mirror_box():
    """Test scene for LONG ray lineages (build-defined): a closed box of six inward-facing perfect mirrors
    (Glossy 1.0: the rotation angles are (1 - p) * rv = 0, so `next` is the exact reflection and no ray leaves) whose
    colour 6.2 makes a bounce keep 6.2 / (2 pi) = 98.7 % of the throughput -- a lineage takes several hundred
    traceSteps before nearZero ends it -- around a small emissive sphere.  The camera of initial_camera() is inside."""
    spheres = np.array([sphere((1.0, -1.0, -8.0), 0.6, (1.0, 0.9, 0.8), 10.0, MATTE, 1.0)], dtype=SPHERE_DTYPE)
    c, g = (6.2, 6.2, 6.2), GLOSSY
    planes = np.array([
        plane((0.0, -4.0, 0.0), (0.0, 1.0, 0.0), c, 0.0, g, 1.0), plane((0.0, 4.0, 0.0), (0.0, -1.0, 0.0), c, 0.0, g, 1.0),
        plane((-6.0, 0.0, 0.0), (1.0, 0.0, 0.0), c, 0.0, g, 1.0), plane((8.0, 0.0, 0.0), (-1.0, 0.0, 0.0), c, 0.0, g, 1.0),
        plane((0.0, 0.0, -14.0), (0.0, 0.0, 1.0), c, 0.0, g, 1.0), plane((0.0, 0.0, 2.0), (0.0, 0.0, -1.0), c, 0.0, g, 1.0),
    ], dtype=PLANE_DTYPE)
    return spheres, planes


def screen_pixels(width, height):
    """screenPixels (src/Util.hs:209-210): Matrix (V2 Int), V2 x y at index (Z :. y :. x)."""
    ys, xs = np.meshgrid(np.arange(height, dtype=np.int64), np.arange(width, dtype=np.int64), indexing="ij")
    return np.ascontiguousarray(xs), np.ascontiguousarray(ys)


def sphere_field(n_spheres, seed=0, glass_fraction=0.0):
    """A seeded random field of n_spheres small spheres in front of initial_camera(), between main_scene()'s floor and ceiling,
    with a back wall and a side wall: 4 planes.  The field is a layer about 0.5 spheres per unit volume dense, as wide and
    deep as it needs to be (10 units for 1 000 spheres, 340 for 10^6); radii 0.1 .. 0.45; matte and glossy, 2 % of them
    emissive; glass_fraction of them GLASS (build-defined: render Streams only).  For BVH scenes (ptmi_set_scene_bvh) --
    tests and tools/bvh_bench.py.  -> (spheres, planes)"""
    rng = np.random.default_rng(seed)
    n = int(n_spheres)
    y0, y1 = -2.8, 14.8
    w = float(np.sqrt(max(n, 1) / (0.5 * (y1 - y0))))
    s = np.zeros(n, dtype=SPHERE_DTYPE)
    s["position"][:, 0] = 1.0 + (rng.random(n, dtype=np.float32) - 0.5) * w
    s["position"][:, 1] = y0 + rng.random(n, dtype=np.float32) * (y1 - y0)
    s["position"][:, 2] = -6.0 - rng.random(n, dtype=np.float32) * w
    s["radius"] = 0.1 + 0.35 * rng.random(n, dtype=np.float32)
    s["color"] = 0.2 + 0.75 * rng.random((n, 3), dtype=np.float32)
    s["illuminance"] = np.where(rng.random(n) < 0.02, 50.0 + 400.0 * rng.random(n), 0.0).astype(np.float32)
    glossy = rng.random(n) < 0.3
    s["brdf_tag"] = np.where(glossy, GLOSSY, MATTE)
    s["brdf_param"] = np.where(glossy, 0.6 + 0.4 * rng.random(n), 0.5 + 0.5 * rng.random(n)).astype(np.float32)
    if glass_fraction > 0.0:
        glass = rng.random(n) < glass_fraction
        s["brdf_tag"][glass] = GLASS
        s["brdf_param"][glass] = 1.5
        s["color"][glass] = (0.95, 0.95, 0.95)
        s["illuminance"][glass] = 0.0
    planes = np.array([
        plane((0.0, -3.0, 0.0), (0.0, 1.0, 0.0), (0.43, 0.95, 0.5), 0.0, MATTE, 1.5),
        plane((0.0, 15.0, 0.0), (0.0, -1.0, 0.0), (0.26, 0.68, 0.88), 0.0, GLOSSY, 0.9),
        plane((0.0, 0.0, -6.0 - w - 4.0), (0.0, 0.0, 1.0), (0.9, 0.9, 0.9), 2.0, MATTE, 1.0),
        plane((1.0 - 0.5 * w - 4.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.8, 0.5, 0.4), 0.0, GLOSSY, 0.7),
    ], dtype=PLANE_DTYPE)
    return s, planes


def triangles_of(vertices, faces, material):
    """TRIANGLE_DTYPE records for faces (k x 3 vertex indices into vertices, k x 3 floats) with one material (color, illuminance,
    brdf_tag, brdf_param)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = np.zeros(len(f), dtype=TRIANGLE_DTYPE)
    t["v0"], t["v1"], t["v2"] = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    color, illuminance, brdf_tag, brdf_param = material
    t["color"] = color
    t["illuminance"] = illuminance
    t["brdf_tag"] = brdf_tag
    t["brdf_param"] = brdf_param
    return t


def triangle_vertices(triangles):
    """The vertices of TRIANGLE_DTYPE records as Context.update_mesh_vertices takes them -> (n, 3, 3) float32, [k] = (v0, v1, v2)"""
    t = np.asarray(triangles, dtype=TRIANGLE_DTYPE).reshape(-1)
    return np.ascontiguousarray(np.stack([t["v0"], t["v1"], t["v2"]], axis=1), dtype=np.float32)


def with_vertices(triangles, v):
    """A copy of the triangles with the vertices v ((n, 3, 3) or (n, 9), as triangle_vertices gives them); materials kept"""
    t = np.array(triangles, dtype=TRIANGLE_DTYPE, copy=True).reshape(-1)
    v = np.asarray(v, np.float32).reshape(len(t), 3, 3)
    t["v0"], t["v1"], t["v2"] = v[:, 0], v[:, 1], v[:, 2]
    return t


def displaced(v, amount, kind="wave", centre=(1.0, 3.0, -16.0), radius=3.0, seed=0):
    """Vertices (as triangle_vertices gives them) with those of mesh_room's icosphere -- everything within 1.5 radii of its centre --
    moved along their own direction from the centre by up to amount * radius: kind "wave" a smooth wave over the sphere, kind "noise" a
    value per vertex.  The displacement is a function of the vertex's POSITION (and the seed), so a vertex shared by several
    triangles, or by a duplicate of a triangle, stays shared.  -> float32, the shape of v; tests and tools/mesh_refit_bench.py"""
    a = np.asarray(v, np.float32)
    p = a.reshape(-1, 3).astype(np.float64)
    rel = p - np.asarray(centre, np.float64)
    dist = np.linalg.norm(rel, axis=1)
    inside = (dist < 1.5 * radius) & (dist > 0)
    unit = rel / np.where(dist > 0, dist, 1.0)[:, None]
    if kind == "wave":
        f = np.sin(5.0 * unit[:, 0] + 0.7 * seed) * np.cos(4.0 * unit[:, 1]) + 0.5 * np.sin(7.0 * unit[:, 2] + 1.3 * seed)
        f = f / 1.5
    elif kind == "noise":
        h = np.sin(p @ np.array([12.9898, 78.233, 37.719]) + 0.61 * seed) * 43758.5453
        f = 2.0 * (h - np.floor(h)) - 1.0
    else:
        raise ValueError("kind is 'wave' or 'noise'")
    out = np.where(inside[:, None], p + unit * (amount * radius * f)[:, None], p)
    return np.ascontiguousarray(out.astype(np.float32).reshape(a.shape))


def sphere_geometry(spheres):
    """The geometry of SPHERE_DTYPE records as Context.update_spheres takes it -> (n, 4) float32, [k] = (x, y, z, radius)"""
    s = np.asarray(spheres, dtype=SPHERE_DTYPE).reshape(-1)
    return np.ascontiguousarray(np.concatenate([s["position"], s["radius"][:, None]], axis=1), dtype=np.float32).reshape(-1, 4)


def with_sphere_geometry(spheres, g):
    """A copy of the spheres with the geometry g ((n, 4), as sphere_geometry gives it); materials kept"""
    s = np.array(spheres, dtype=SPHERE_DTYPE, copy=True).reshape(-1)
    g = np.asarray(g, np.float32).reshape(len(s), 4)
    s["position"], s["radius"] = g[:, :3], g[:, 3]
    return s


def displaced_spheres(g, amount, kind="wave", seed=0):
    """Sphere geometry (as sphere_geometry gives it) with every centre moved by up to `amount` (a length), radii kept: kind "wave" a
    smooth wave along y over x and z, kind "noise" an independent seeded offset per sphere and axis.  -> (n, 4) float32; tests and
    tools/bvh_update_bench.py"""
    out = np.array(g, np.float32, copy=True).reshape(-1, 4)
    p = out[:, :3].astype(np.float64)
    if kind == "wave":
        p[:, 1] += amount * np.sin(0.7 * p[:, 0] + 0.9 * seed) * np.cos(0.5 * p[:, 2])
    elif kind == "noise":
        p += amount * (2.0 * np.random.default_rng(seed).random(p.shape) - 1.0)
    else:
        raise ValueError("kind is 'wave' or 'noise'")
    out[:, :3] = p.astype(np.float32)
    return np.ascontiguousarray(out)


def load_obj(path_or_text, material):
    """A minimal Wavefront OBJ reader: `v x y z` and `f a b c ...` lines only (1-based indices, negative ones counted back from the
    last vertex read, `a/b/c` forms use the position index); polygons are fan-triangulated (a b c, a c d, ...); every other line is
    ignored.  path_or_text: a file name, or the text itself when it holds a newline.  -> TRIANGLE_DTYPE records with `material`."""
    text = path_or_text
    if "\n" not in path_or_text:
        with open(path_or_text) as fh:
            text = fh.read()
    verts, faces = [], []
    for line in text.splitlines():
        parts = line.split("#", 1)[0].split()
        if not parts:
            continue
        if parts[0] == "v" and len(parts) >= 4:
            verts.append([float(x) for x in parts[1:4]])
        elif parts[0] == "f" and len(parts) >= 4:
            idx = []
            for p in parts[1:]:
                k = int(p.split("/")[0])
                idx.append(k - 1 if k > 0 else len(verts) + k)
            if any(i < 0 or i >= len(verts) for i in idx):
                raise ValueError("OBJ face refers to a vertex that does not exist: %r" % line)
            for j in range(1, len(idx) - 1):
                faces.append((idx[0], idx[j], idx[j + 1]))
    return triangles_of(np.array(verts, np.float32).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3), material)


def icosphere(subdivisions):
    """The unit icosphere: an icosahedron whose faces are split into 4 `subdivisions` times, vertices pushed onto the sphere; faces
    counter-clockwise seen from outside.  20 * 4^subdivisions faces.  -> (vertices k x 3 float64, faces m x 3)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(int(subdivisions)):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v, f = np.array(verts), np.array(f, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    inward = np.einsum("ij,ij->i", n, v[f[:, 0]]) < 0
    f[inward] = f[inward][:, [0, 2, 1]]                 # counter-clockwise seen from outside
    return v, f


def mesh_room(subdivisions=2, n_spheres=8, seed=0):
    """A closed room of triangles (12: floor, glowing ceiling, four walls, inward-facing) with an emissive triangle light under the ceiling,
    n_spheres spheres inside, and an icosphere mesh of 20 * 4^subdivisions triangles (2 -> 320, 4 -> 5 120, 6 -> 81 920, 8 -> 1.3 M)
    in front of initial_camera().  No planes.  For mesh scenes (ptmi_set_scene_mesh) -- tests and tools/mesh_bench.py.
    -> (spheres, triangles, planes)"""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1, z0, z1 = -12.0, 14.0, -3.0, 15.0, -30.0, 8.0
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    # the six faces, each a quad (a, b, c, d), turned below to face into the room
    quads = [((0, 1, 5, 4), (0.43, 0.95, 0.5), 0.0, MATTE, 1.0),        # floor (y0), normal +y
             ((3, 7, 6, 2), (0.9, 0.9, 0.85), 2.0, MATTE, 1.0),         # ceiling (y1), normal -y, glowing
             ((0, 3, 2, 1), (0.9, 0.9, 0.9), 0.0, MATTE, 1.0),          # back (z0), normal +z
             ((4, 5, 6, 7), (0.8, 0.8, 0.8), 0.0, MATTE, 0.8),          # front (z1), normal -z
             ((0, 4, 7, 3), (0.8, 0.5, 0.4), 0.0, GLOSSY, 0.7),         # left (x0), normal +x
             ((1, 2, 6, 5), (0.4, 0.5, 0.8), 0.0, MATTE, 0.9)]          # right (x1), normal -x
    tris = []
    for (a, b, cc, d), col, il, tag, p in quads:
        tris.append(triangle(c[a], c[b], c[cc], col, il, tag, p))
        tris.append(triangle(c[a], c[cc], c[d], col, il, tag, p))
    centre = np.array([(x0 + x1) / 2, (y0 + y1) / 2, (z0 + z1) / 2])
    for k, (v0, v1, v2, *rest) in enumerate(tris):             # every wall faces into the room
        n = np.cross(np.subtract(v1, v0), np.subtract(v2, v0))
        if np.dot(n, centre - np.array(v0)) < 0:
            tris[k] = (v0, v2, v1, *rest)
    # the light: one triangle facing down, just under the ceiling
    tris.append(triangle((-2.0, 14.5, -14.0), (4.0, 14.5, -14.0), (1.0, 14.5, -8.0), (1.0, 0.95, 0.9), 40.0, MATTE, 1.0))
    room = np.array(tris, dtype=TRIANGLE_DTYPE)
    v, f = icosphere(subdivisions)
    mesh = triangles_of(v * 3.0 + np.array([1.0, 3.0, -16.0]), f, ((0.85, 0.75, 0.4), 0.0, GLOSSY, 0.8))
    s = np.zeros(int(n_spheres), dtype=SPHERE_DTYPE)
    s["position"][:, 0] = -8.0 + 18.0 * rng.random(len(s))
    s["position"][:, 1] = -2.0 + 6.0 * rng.random(len(s))
    s["position"][:, 2] = -26.0 + 16.0 * rng.random(len(s))
    s["radius"] = 0.5 + 0.8 * rng.random(len(s))
    s["color"] = 0.2 + 0.75 * rng.random((len(s), 3))
    s["illuminance"] = np.where(np.arange(len(s)) % 4 == 0, 30.0, 0.0)
    s["brdf_tag"] = np.where(np.arange(len(s)) % 3 == 0, GLOSSY, MATTE)
    s["brdf_param"] = 0.8
    return s, np.concatenate([room, mesh]), np.zeros(0, dtype=PLANE_DTYPE)
