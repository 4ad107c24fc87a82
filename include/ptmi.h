/*
 * ptmi.h -- C ABI of libptmi, the MI355X-native replacement for the one compute
 * call of robbert-vdh/haskell-path-tracer:
 *
 *     dewit = runN (render config) screenPixels            (app/Main.hs:190)
 *     \c (it, acc) -> (it + 1, dewit (scalar c) acc)        (app/Main.hs:191)
 *
 * plus the two array programs that create / replace the RNG planes
 * (`run <$> initialOutput` app/Main.hs:155,306 ; `run <$> reseed ...` :231).
 *
 * The reference has no FFI for this path (the boundary is a Haskell closure,
 * `type CompiledFunction`, app/Main.hs:83-84); these entry points are what a
 * `foreign import ccall` module replacing line 190 binds (INTEGRATION.md shows it).
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns 0 (PTMI_OK) or a negative
 *     PTMI_E* code; ptmi_last_error(ctx) holds the message.  Nothing throws or aborts.
 *     (The reference surfaces failures as Haskell exceptions out of runN; the Haskell
 *     wrapper turns a non-zero code into throwIO.)
 *   - A RenderResult = Matrix (Color, SFC32) (src/Scene/Objects.hs:36) is SEVEN planes,
 *     row-major [rows][width], x fastest (src/Util.hs:213-214): r, g, b (binary32) and
 *     the SFC32 state a, b, c, counter (uint32) -- Accelerate's struct-of-arrays layout
 *     as seen through A.toVectors (app/Main.hs:350).
 *   - The colour planes hold a SUM over samples; averaging is the presenter's job
 *     (app/assets/fs.glsl:12).
 *   - A context may be entered from any OS thread (app/Main.hs:178-180 forks two bound
 *     threads); calls on one context are serialised by an internal mutex.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_VERSION 600   /* 0.6.0: the chained closure (ptmi_render1_chained, ptmi_chain_*: device residency behind compileFor's pure type), PTMI_ESTALE,
                            * options 14 and 15, PTMI_FORM_PIXEL; ordered passes hand off with release / acquire per region; ptmi_build_id names the
                            * compiled code, not the source text.  0.5.0: ptmi_build_id; ptmi_debug_counters writes 64 words again (as in 0.3) and ptmi_debug_counters_n takes a
                            * capacity; option 13 and ptmi_stream_tickets; the stream form's overflow streams grow instead of dropping children;
                            * no option is read from the environment any more.  (0.4.0: options 8-12, ptmi_stream_schedule.)
                            * Added without a version bump: the bounding-volume-hierarchy scene (ptmi_set_scene_bvh, ptmi_group_set_scene_bvh,
                            * ptmi_bvh_layout, ptmi_bvh_node, PTMI_MAX_BVH_*) and ptmi_eval_check_hit; the mesh scene (ptmi_set_scene_mesh,
                            * ptmi_group_set_scene_mesh, ptmi_mesh_layout, ptmi_triangle, PTMI_MAX_MESH_TRIANGLES); moving a mesh scene's
                            * vertices (ptmi_update_mesh_vertices, ptmi_update_mesh_vertices_device, ptmi_group_update_mesh_vertices,
                            * ptmi_mesh_refit_layout, ptmi_mesh_read_layout); new triangles for a mesh scene, built on the device
                            * (ptmi_set_mesh_triangles, ptmi_set_mesh_triangles_device, ptmi_group_set_mesh_triangles,
                            * ptmi_mesh_layout_morton); moving and replacing a BVH or mesh scene's spheres on the device
                            * (ptmi_update_spheres, ptmi_update_spheres_device, ptmi_set_bvh_spheres, ptmi_set_bvh_spheres_device,
                            * ptmi_group_update_spheres, ptmi_group_set_bvh_spheres, ptmi_bvh_refit_layout, ptmi_bvh_layout_morton,
                            * ptmi_bvh_read_layout); the spatial device build of a sphere hierarchy (option 17 = PTMI_OPT_BVH_DEVICE_BUILD,
                            * PTMI_BVH_BUILD_*, ptmi_bvh_layout_spatial); the ray queries on device-resident rays (ptmi_trace_rays_device,
                            * ptmi_occluded_device); paths along device-resident rays (ptmi_trace_paths_device,
                            * ptmi_trace_paths_indexed_device, ptmi_path_seeds_device); those paths one bounce at a time and the list
                            * of live rays (ptmi_bounce_rays_device, ptmi_bounce_rays_indexed_device, ptmi_live_rays_device); the
                            * nearest-primitive query (ptmi_nearest_device, ptmi_nearest_indexed_device, ptmi_nearest). */

/* ---- error codes ------------------------------------------------------------ */
enum {
    PTMI_OK        =  0,
    PTMI_EINVAL    = -1,   /* bad argument (null pointer, empty scene, size <= 0 ...)        */
    PTMI_ENODEVICE = -2,   /* no HIP device / device index out of range                       */
    PTMI_EHIP      = -3,   /* a HIP runtime call failed; message in ptmi_last_error          */
    PTMI_ENOMEM    = -4,   /* device or host allocation failed                                */
    PTMI_ESTATE    = -5,   /* call order violated (render before set_scene / resize ...)     */
    PTMI_ELIMIT    = -6,   /* scene larger than PTMI_MAX_PRIMITIVES (PTMI_MAX_BVH_* for ptmi_set_scene_bvh); an image of more than 2^40 pixels (or beyond the stream form's limits) */
    PTMI_ESTALE    = -7    /* a token names no state this context holds (released, consumed, or another context's) */
};

/* data Algorithm = Streams | Inline                       (src/Scene/Trace.hs:68) */
enum { PTMI_STREAMS = 0, PTMI_INLINE = 1 };

/* data Brdf = Matte Float | Glossy Float                 (src/Scene/Objects.hs:77-87)
 * PTMI_GLASS is a build-defined EXTENSION (parameter = index of refraction): a hit spawns a reflection and a
 * refraction ray.  The reference only announces such materials (src/Scene/Trace.hs:109-118, :306-307, :327-328),
 * so GLASS has no reference semantics; it is accepted by PTMI_STREAMS only (Inline cannot split rays,
 * src/Scene/Trace.hs:62-67).  On one GPU a scene with GLASS is rendered by the per-pixel TREE WALK (deterministic, bit-exact
 * against the oracle: one adder per colour word); one PART of a partitioned image at >= 256 samples per call by the stream ("wavefront")
 * form -- BASELINE configs[4]'s path: faster where the job is bounded by its slowest part, colours through float atomics in no defined
 * order.  PTMI_OPT_STREAMS_FORM chooses explicitly.  See DESIGN.md 5.5.
 * What a GLASS hit does, for a ray of direction d that meets the normal n at the point p with the generator state `seed`:
 *   (rv, seed') = genVec seed                       -- drawn and discarded, as for every material (src/Scene/Trace.hs:402)
 *   dn = d . n ; cosi = -dn ; eta = 1 / ior ; k = 1 - (eta*eta) * (1 - cosi*cosi)
 *   reflection = d - (2*dn) *^ n                     -- the Glossy formula (src/Scene/Trace.hs:421-422)
 *   r0 = ((1-ior)/(1+ior))^2 ; m = 1 - cosi ; R = r0 + (1-r0) * (((m*m)*(m*m))*m)   -- Schlick
 *   k < 0 (total internal reflection):  R = 1, refraction = reflection
 *   else refraction = eta *^ d + (eta*cosi - sqrt k) *^ n
 *   child 0 = (p + reflection ^* epsilon, reflection), throughput * (color ^* R),     seed'
 *   child 1 = (p + refraction ^* epsilon, refraction), throughput * (color ^* (1-R)), seed' advanced one more draw
 * Back faces are culled by distanceTo, so a refracted ray never meets the far side of its own sphere. */
enum { PTMI_MATTE = 0, PTMI_GLOSSY = 1, PTMI_GLASS = 2 };

#define PTMI_MAX_PRIMITIVES 1024   /* spheres + planes staged in LDS per workgroup */
#define PTMI_MAX_BVH_SPHERES (1 << 22)   /* ptmi_set_scene_bvh: spheres in the hierarchy */
#define PTMI_MAX_BVH_PLANES  64          /* ... planes, folded linearly after the spheres */
#define PTMI_BVH_MAX_DEPTH   24          /* levels of inner nodes (the root is level 0); the device keeps one stack entry per level */
#define PTMI_BVH_LEAF_MAX    4           /* spheres per leaf */
#define PTMI_MAX_MESH_TRIANGLES (1 << 22) /* ptmi_set_scene_mesh: triangles in the second hierarchy (spheres and planes as for BVH scenes) */

/* ---- scene types: field order = src/Scene/Objects.hs ------------------------ */
typedef struct ptmi_sphere {       /* data Sphere   Objects.hs:126-131, Material :90-100 */
    float   position[3];
    float   radius;
    float   color[3];
    float   illuminance;
    int32_t brdf_tag;              /* PTMI_MATTE | PTMI_GLOSSY (| PTMI_GLASS, extension) */
    float   brdf_param;
} ptmi_sphere;                     /* 10 words */

typedef struct ptmi_plane {        /* data Plane    Objects.hs:103-108 */
    float   position[3];
    float   direction[3];          /* the normal; used as stored (Intersection.hs:64) */
    float   color[3];
    float   illuminance;
    int32_t brdf_tag;
    float   brdf_param;
} ptmi_plane;                      /* 12 words */

/* One inner node of the sphere hierarchy of ptmi_set_scene_bvh (ptmi_bvh_layout returns them; node 0 is the root): the boxes of
 * BOTH children, as centre and half extent, so that one 64-byte fetch tests two boxes.  ref[c] >= 0: child c is inner node ref[c];
 * ref[c] < 0: child c is a leaf of ((-1 - ref[c]) & 255) spheres starting at position (-1 - ref[c]) >> 8 of the
 * leaf order; -1 is an empty child.  inv_2r[c] = 1 / (2 r_min), r_min the smallest |radius| under child c (+inf when it is 0): the traversal's margin for
 * rounding in the sphere test depends on it (DESIGN.md "BVH scenes").  A child's box holds every sphere under it, each padded
 * (centre +- (|r| (1 + 2^-8) + 2^-20 max(|centre|, |r|))). */
typedef struct ptmi_bvh_node {
    float   center[2][3];
    float   half[2][3];
    int32_t ref[2];
    float   inv_2r[2];
} ptmi_bvh_node;                   /* 16 words */

/* A triangle (extension: the reference has no triangle type).  A bounded, one-sided plane: n = cross(v1 - v0, v2 - v0), the front is
 * counter-clockwise; hit where the plane (v0, n / |n|) is hit (distanceTo @Plane) and the hit point lies inside or on the edges.  A
 * triangle of zero area is never hit.  Material fields as in ptmi_sphere and ptmi_plane. */
typedef struct ptmi_triangle {
    float   v0[3], v1[3], v2[3];
    float   color[3];
    float   illuminance;
    int32_t brdf_tag;
    float   brdf_param;
} ptmi_triangle;                   /* 15 words */

typedef struct ptmi_camera {       /* data Camera   Objects.hs:67-74 */
    float   position[3];
    float   rotation[3];           /* (roll, pitch, yaw) Euler angles */
    int64_t fov;                   /* horizontal field of view, degrees; Haskell Int */
} ptmi_camera;

typedef struct ptmi_stats {
    uint64_t live_bounces;         /* Inline: iterations that took computeRay (Trace.hs:374); Streams: child rays emitted -- since the last reset */
    uint64_t nominal_bounces;      /* pixels x samples x bounce_limit since the last reset                  */
    uint64_t samples;              /* pixels x samples                                                       */
    float    last_render_ms;       /* device time of the last ptmi_render launch(es); 0 unless timing is on */
    uint32_t stream_iterations;    /* Streams: the longest chain of traceSteps any ray lineage took (stream form: of the last sample) */
    uint64_t stream_rays_dropped;  /* Streams with ray splitting: children that found no room -- tree walk: a lane's stack of 16 waiting children full; stream form: the overflow streams full even at 64 rays per pixel (below that the call is redone with longer streams) */
    uint64_t stream_rays_truncated;/* Streams: rays still alive when PTMI_OPT_STREAM_STEP_CAP cut their lineage (the reference has no cap) */
    uint64_t stream_rays_spilled;  /* Streams, stream form: children that found their wave's ring in LDS full and travelled through HBM (nothing is lost) */
    uint64_t stream_rays_overflowed; /* ... of which those that found the wave's spill queue full too and were traced by a later launch (an overflow level) */
} ptmi_stats;

typedef struct ptmi_ctx ptmi_ctx;

/* ---- lifetime ---------------------------------------------------------------- */
int         ptmi_version(void);
/* Which code this binary holds: 16 hex digits of a sha256 over the allocated sections of the objects it was linked from -- host code and
 * the gfx950 code objects (haskell-path-tracer_amd/_build.py: code_id) -- followed by "+<flags>" for a non-default build (ablations,
 * diagnostic builds).  A comment or documentation edit leaves it unchanged; an instruction, a constant or a kernel's name changes it.
 * Every measurement names it (bench.py: binary_build_id; profiles/): a number belongs to the binary that carries the id, and the
 * Python binding refuses a library that does not hold the code the sources beside it compile to.  Never NULL; static storage. */
const char *ptmi_build_id(void);
const char *ptmi_strerror(int code);
/* Create a context on HIP device `device` (>= 0).  Fails with PTMI_ENODEVICE when the
 * machine has no usable GPU: there is NO CPU fallback in this library. */
int         ptmi_create(ptmi_ctx **out, int device);
void        ptmi_destroy(ptmi_ctx *ctx);
/* The message of the calling THREAD's last failed call on `ctx` (ctx NULL: of its last failed ptmi_create); if this thread has not failed on
 * `ctx`, the context's latest message whoever saw it.  The text stays valid until the same thread's next failing call or next ptmi_last_error:
 * threads that share a context never read each other's strings.  A HIP error reported through a return code is taken out of the runtime's
 * own sticky slot (hipGetLastError) -- the caller's next launch check does not find it again -- and an error another library left there
 * is neither mistaken for this library's nor cleared by it.
 * After a failure the context stays usable and consistent: a failed ptmi_set_scene keeps the scene it had; a failed ptmi_resize leaves the
 * context UNSIZED (calls that need planes answer PTMI_ESTATE until a ptmi_resize succeeds; ptmi_group_resize likewise for the group); a
 * render call that fails with PTMI_EHIP / PTMI_ENOMEM half-way leaves the CONTENT of the planes unspecified (re-initialise them), never a
 * dangling pointer.  tests/test_host_sanitized.py walks every failure point under AddressSanitizer. */
const char *ptmi_last_error(const ptmi_ctx *ctx);

/* ---- configuration ----------------------------------------------------------- */
/* mainScene (src/Scene/World.hs:15-77) as run-time data.  Order is kept: checkHit folds
 * over spheres then planes (src/Util.hs:156-158) and ties keep the earlier primitive. */
int ptmi_set_scene(ptmi_ctx *ctx, const ptmi_sphere *spheres, int n_spheres,
                   const ptmi_plane *planes, int n_planes);

/* The same scene semantics (spheres then planes; ties keep the earlier primitive: the render is bit for bit the one ptmi_set_scene
 * would give) for scenes of up to PTMI_MAX_BVH_SPHERES spheres and PTMI_MAX_BVH_PLANES planes: the spheres go into a bounding-volume
 * hierarchy built on the host (ptmi_bvh_layout), the planes stay a linear list.  Hits are found by walking the hierarchy, so a
 * bounce costs about log(n) box tests instead of n sphere tests -- and more than the linear fold for small scenes: opt-in.
 * Fails with PTMI_ELIMIT beyond the limits (0 spheres and 0 planes: PTMI_EINVAL) and with PTMI_EINVAL when a sphere's position,
 * radius or radius^2 is not finite (a box cannot bound a NaN).  Transactional: after a failure the previous scene, of either kind,
 * stays.  ptmi_set_scene afterwards (or before) switches representation.  A BVH scene renders through the per-pixel kernels only:
 * PTMI_OPT_STREAMS_FORM = PTMI_FORM_STREAM, ptmi_set_variant != 0 and the ablation library refuse it with PTMI_EINVAL
 * (PTMI_FORM_AUTO picks the per-pixel form). */
int ptmi_set_scene_bvh(ptmi_ctx *ctx, const ptmi_sphere *spheres, int n_spheres,
                       const ptmi_plane *planes, int n_planes);

/* The hierarchy ptmi_set_scene_bvh builds for these spheres, without a device (pure host code, deterministic): node 0 is the root,
 * order[k] is the original index of the sphere at position k of the leaf order.  `nodes` needs max(1, n_spheres) entries
 * (node_capacity), `order` n_spheres.  Returns the number of nodes; PTMI_ELIMIT beyond PTMI_MAX_BVH_SPHERES or when node_capacity
 * is too small, PTMI_EINVAL for NULL pointers or non-finite sphere data. */
int ptmi_bvh_layout(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order);

/* A MESH scene: a BVH scene (the spheres through ptmi_set_scene_bvh's hierarchy, the planes folded linearly) plus up to
 * PTMI_MAX_MESH_TRIANGLES triangles in a second hierarchy (ptmi_mesh_layout).  checkHit folds over spheres ++ planes ++ triangles:
 * triangle k is primitive n_spheres + n_planes + k, and every tie keeps the earlier primitive, so with no triangles the render is bit
 * for bit the BVH scene's.  Fails with PTMI_ELIMIT beyond the limits (nothing at all: PTMI_EINVAL), with PTMI_EINVAL for non-finite
 * sphere, vertex or material data or a normal whose square does not stay finite, and -- as ptmi_set_scene_bvh -- for the stream form,
 * a variant other than 0 and the ablation library (PTMI_FORM_AUTO picks the per-pixel form); render Inline has no contracted
 * kernel for it.  Transactional: after a failure the previous scene, of any kind, stays. */
int ptmi_set_scene_mesh(ptmi_ctx *ctx, const ptmi_sphere *spheres, int n_spheres, const ptmi_triangle *triangles, int n_triangles,
                        const ptmi_plane *planes, int n_planes);

/* The triangle hierarchy ptmi_set_scene_mesh builds (pure host code, deterministic), in ptmi_bvh_node form: inv_2r is 0, each
 * triangle's box is padded as DESIGN.md 5.8 says and order[k] is the original index of the triangle at position k of the leaf order.
 * Triangles of zero area are in no leaf: the return value's order has n_kept entries (*n_kept, may be NULL).  `nodes` needs
 * max(1, n_triangles) entries, `order` n_triangles.  Returns the number of nodes, or PTMI_ELIMIT / PTMI_EINVAL as ptmi_bvh_layout. */
int ptmi_mesh_layout(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept);

/* Move the vertices of the current MESH scene without building anything on the host: the triangle hierarchy keeps its topology (child
 * references, leaf order) and is REFIT on the device -- new boxes, bottom-up, one launch per level -- and both copies of the triangle
 * records are rewritten.  `vertices` holds 9 floats per triangle, v0 v1 v2, in the index order of the `triangles` given to
 * ptmi_set_scene_mesh, in host memory (ptmi_update_mesh_vertices: staged to the device, then the same path) or in device memory of the
 * context's device (ptmi_update_mesh_vertices_device; read on the context's stream).  Materials, spheres and planes stay as set.
 *   - Renders equal a fresh scene: after an update every render (all seven planes) and ptmi_eval_check_hit equal, bit for bit, those of
 *     a context given ptmi_set_scene_mesh with the moved triangles: the device derives each record (v0, nx) (v1, ny) (v2, nz) by
 *     ptmi_set_scene_mesh's own operations (edges, cross product in linear's component order, (nx^2 + ny^2) + nz^2, IEEE square root,
 *     three IEEE divisions, each f32 operation rounded on its own), and check_hit returns the fold over spheres ++ planes ++ triangles
 *     whatever hierarchy bounds the triangles.  The refitted boxes are those of ptmi_mesh_refit_layout, bit for bit.
 *   - A failed update leaves the scene as it was: PTMI_ESTATE when the current scene is not a mesh scene; PTMI_EINVAL for a NULL
 *     pointer, for an n_triangles other than the scene's, for a non-finite vertex, edge, normal or normal^2 (ptmi_set_scene_mesh's
 *     conditions), and when a triangle that had ZERO AREA WHEN THE SCENE WAS SET would gain area -- it is in no leaf, the topology
 *     cannot serve it: the message names the triangle, set the scene again.  The new vertices are validated by a kernel that writes
 *     nothing of the scene, and the update is written into a second copy of the scene's mesh block that replaces the first only when
 *     every launch is out: after PTMI_EHIP too the scene is the one before the call.
 *   - A triangle in a leaf that collapses to zero area is accepted: it stays in its leaf with a NaN normal (never hit), its vertices
 *     still count for its box.
 *   - One host synchronisation per call (the verdict and the new box of the leaf triangles' vertices are read back together); the
 *     writing kernels then run on the context's stream like a render.  Neither the old nor the new vertices are needed on the host.
 * The topology is the one built for the scene AS SET: after large deformations the refitted boxes overlap more than a fresh build's
 * and renders get slower, never different (DESIGN.md 5.8 has the measurements); call ptmi_set_scene_mesh again then, or
 * ptmi_set_mesh_triangles[_device] when the triangles live on the device or their count or connectivity changes.  Moving
 * or replacing the spheres is ptmi_update_spheres / ptmi_set_bvh_spheres (below); moving planes, or changing the materials of planes
 * or triangles, is a scene call. */
int ptmi_update_mesh_vertices(ptmi_ctx *ctx, const float *vertices, int n_triangles);          /* host memory   */
int ptmi_update_mesh_vertices_device(ptmi_ctx *ctx, const float *d_vertices, int n_triangles); /* device memory */

/* The device refit's specification and CPU twin (pure host code): `nodes` (n_nodes of them) and `order` (n_kept entries) as
 * ptmi_mesh_layout returned them for the scene as set, `triangles` the moved ones.  Overwrites center and half of every child in
 * place with ptmi_mesh_layout's own arithmetic -- a leaf child's box is the union of its triangles' padded vertex boxes, an inner
 * child's the union of that node's two stored boxes, one sweep from the last node to node 0 (children have larger ids than their
 * parent) -- and leaves ref and inv_2r (0) alone.  It depends on the topology and the current vertices only: unchanged vertices
 * give ptmi_mesh_layout's nodes back byte for byte, and so does moving away and back.  PTMI_EINVAL, with nothing written, for nodes
 * and order that do not belong together (a wrong n_nodes or n_kept), non-finite vertex data, or a triangle in no leaf that has area. */
int ptmi_mesh_refit_layout(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order, int n_kept);

/* Replace the TRIANGLES of the current MESH scene -- another count, another connectivity, a fresh mesh -- without building anything on
 * the host: `triangles` holds n_triangles records (0 .. PTMI_MAX_MESH_TRIANGLES), geometry and materials, in host memory
 * (ptmi_set_mesh_triangles: staged to the device, then the same path) or in device memory of the context's device
 * (ptmi_set_mesh_triangles_device; read on the context's stream).  Spheres, their hierarchy and planes stay as set.
 *   - The result is a fresh scene: every render (all seven planes, Inline and Streams, GLASS included), ptmi_eval_check_hit and a later
 *     ptmi_update_mesh_vertices[_device] equal, bit for bit, those of a context given ptmi_set_scene_mesh(spheres, new triangles, planes).
 *     Records and materials are derived on the device by ptmi_set_scene_mesh's own operations, and check_hit returns the fold over
 *     spheres ++ planes ++ triangles whatever hierarchy bounds the triangles.
 *   - The hierarchy is NOT ptmi_mesh_layout's: the leaf order ascends by (Morton key of the centroid within the box of the kept
 *     triangles' vertices, index) -- a radix sort on the device -- and the topology is a function of the kept count alone (equal-count
 *     splits, ptmi_mesh_layout's depth); the boxes are the refit's over it.  ptmi_mesh_layout_morton is its specification and host twin:
 *     ptmi_mesh_read_layout afterwards returns exactly its nodes and order.
 *   - Refusals leave the scene as it was: PTMI_ESTATE when the current scene is not a mesh scene; PTMI_ELIMIT beyond the limit;
 *     PTMI_EINVAL for NULL with n > 0, a negative n, 0 triangles in a scene without spheres and planes, and for everything
 *     ptmi_set_scene_mesh refuses in a triangle -- a non-finite vertex, colour, illuminance or brdf_param, non-finite edges, normal or
 *     normal^2, an unknown brdf_tag: the message names the triangle.  The new data is validated by a kernel that writes nothing of the
 *     scene; the new blocks are written aside and replace the old ones only when all of it is through: after PTMI_EHIP / PTMI_ENOMEM
 *     too the scene is the one before the call.
 *   - A triangle of zero area keeps its index and material, has a NaN normal and is in no leaf, as with ptmi_set_scene_mesh; a later
 *     update that would give it area is refused.
 *   - Two host synchronisations per call: one reads the verdict, the kept count, the box and whether any triangle is GLASS, together;
 *     one drains the stream before the old blocks and the sort's scratch are freed.  Neither the old nor the new triangles are needed
 *     on the host.
 * The Morton order with equal-count splits is another tree than ptmi_mesh_layout's longest-axis median splits.  Measured (DESIGN.md 5.8,
 * profiles/mesh_build_bench.json): the call takes 1.5 / 17 ms from device memory against ptmi_set_scene_mesh's 16 / 426 ms at 82k / 1.3M
 * triangles; a 1080p render over this tree takes x 0.80 / 0.96 of the time over ptmi_mesh_layout's at 1.3k / 82k triangles and x 1.15 at
 * 1.3M: ptmi_set_scene_mesh remains the call for a static mesh. */
int ptmi_set_mesh_triangles(ptmi_ctx *ctx, const ptmi_triangle *triangles, int n_triangles);          /* host memory   */
int ptmi_set_mesh_triangles_device(ptmi_ctx *ctx, const ptmi_triangle *d_triangles, int n_triangles); /* device memory */

/* The hierarchy ptmi_set_mesh_triangles builds, without a device (pure host code, deterministic): ptmi_mesh_layout's signature, return
 * values and refusals; ptmi_mesh_refit_layout accepts the result and leaves it byte-identical. */
int ptmi_mesh_layout_morton(const ptmi_triangle *triangles, int n_triangles, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept);

/* The triangle hierarchy the context's mesh scene holds NOW, copied back from the device (test and diagnostic surface, like
 * ptmi_bvh_layout / ptmi_eval_check_hit): after updates, ptmi_mesh_refit_layout's nodes bit for bit.  `nodes` needs the scene's node
 * count (node_capacity; PTMI_ELIMIT when too small), `order` its kept triangles (*n_kept, may be NULL).  With `nodes` and `order` both
 * NULL nothing is copied: the return value and *n_kept say what to allocate.  Returns the number of nodes; PTMI_ESTATE when the
 * current scene is not a mesh scene.  Synchronises the context's stream. */
int ptmi_mesh_read_layout(ptmi_ctx *ctx, ptmi_bvh_node *nodes, int node_capacity, int32_t *order, int *n_kept);

/* MOVE the spheres of the current BVH or MESH scene (both keep them in one sphere hierarchy) and refit that hierarchy on the device, without a
 * scene call.  geometry: 4 floats per sphere -- x, y, z, radius -- in the index order of the scene as set, in host memory
 * (ptmi_update_spheres: staged to the device, then the same path) or in device memory of the context's device (ptmi_update_spheres_device;
 * read on the context's stream).  The count, the materials, the planes and the triangles stay; so do the hierarchy's topology and leaf order.
 *   - Every later render (all seven planes, Inline and Streams, both seed rules, the GLASS tree walk) and every ptmi_eval_check_hit result
 *     equals, bit for bit, that of a context given ptmi_set_scene_bvh / ptmi_set_scene_mesh with the moved spheres: the device writes each
 *     (centre, radius * radius) record by the scene calls' own operation, and check_hit returns the fold over ALL spheres whatever
 *     hierarchy bounds them.  The refitted boxes and inv_2r are those of ptmi_bvh_refit_layout, bit for bit.
 *   - A failed update leaves the scene as it was: PTMI_ESTATE for a linear or unset scene; PTMI_EINVAL for a NULL pointer with
 *     n_spheres > 0, for an n_spheres other than the scene's, and for a non-finite position, radius or radius^2 (ptmi_last_error names the
 *     smallest offending index).  Validation is a kernel that writes nothing of the scene; the update is written into second copies of the
 *     hierarchy and scene blocks that replace the first only when every launch is out: after PTMI_EHIP / PTMI_ENOMEM the scene is the one
 *     before the call.
 *   - ONE host synchronisation per update (the verdict and the box of the centres, read together); the writing kernels run behind it on
 *     the context's stream.
 * The topology is not rebuilt: after large displacements the boxes overlap more and renders get slower, never different; call
 * ptmi_set_bvh_spheres[_device] or the scene call again then. */
int ptmi_update_spheres(ptmi_ctx *ctx, const float *geometry, int n_spheres);          /* host memory   */
int ptmi_update_spheres_device(ptmi_ctx *ctx, const float *d_geometry, int n_spheres); /* device memory */

/* REPLACE the spheres of the current BVH or MESH scene -- another count (0 .. PTMI_MAX_BVH_SPHERES), new materials -- and build their
 * hierarchy on the device.  spheres: full ptmi_sphere records in host memory (ptmi_set_bvh_spheres: staged, then the same path) or in
 * device memory (ptmi_set_bvh_spheres_device; read on the context's stream).  Planes and triangles stay as set.
 *   - Every later render and ptmi_eval_check_hit result equals, bit for bit, that of a context given ptmi_set_scene_bvh /
 *     ptmi_set_scene_mesh with the new spheres: the packed scene block is rebuilt on the device for the new count, sphere rows and
 *     materials by the scene calls' own operations, the planes' and triangles' rows copied to their new offsets.
 *   - The hierarchy is NOT ptmi_bvh_layout's: the leaf order ascends by (Morton key of the centre within the f32 box of all centres, index)
 *     -- every sphere is kept, radius 0 too -- the topology is a function of the count alone (equal-count splits, ptmi_bvh_layout's
 *     depth), the boxes are the refit's over it.  ptmi_bvh_layout_morton is its specification and host twin: ptmi_bvh_read_layout
 *     afterwards returns exactly its nodes and order.
 *   - Refusals leave the scene as it was: PTMI_ESTATE for a linear or unset scene; PTMI_ELIMIT beyond the limit; PTMI_EINVAL for a NULL
 *     pointer with n_spheres > 0, a negative n_spheres, 0 spheres in a scene with nothing else, a non-finite position, radius, radius^2,
 *     colour, illuminance or brdf_param, or an unknown brdf_tag (the smallest offending index is named).  Validation is a kernel that
 *     writes nothing of the scene; new blocks are written aside and swapped in only when every launch is out: after PTMI_EHIP /
 *     PTMI_ENOMEM the scene is the one before the call.  A GLASS sphere under PTMI_SEED_FROM_RESULT is refused where
 *     ptmi_set_mesh_triangles' GLASS is: by the next render Streams, not here.
 *   - TWO host synchronisations per call: the verdict, box and GLASS flag; then the drained stream before the old blocks go.
 *   - Under PTMI_OPT_BVH_DEVICE_BUILD = PTMI_BVH_BUILD_SPATIAL everything above holds but the tree: it is ptmi_bvh_layout_spatial's, bit for
 *     bit, built on the device top-down, two launches per level, its nodes numbered breadth-first by a prefix sum in id order (no atomics).
 *     The host reads 25 words back in between -- the node count of every level, which size the hierarchy, the refit's launches and a later
 *     ptmi_update_spheres -- so the call makes THREE host synchronisations.
 * Measured (tools/bvh_update_bench.py, profiles/bvh_update_bench.json; an MI355X at 2.4 GHz), 1 020 / 10^5 / 10^6 spheres, from device
 * memory: ptmi_update_spheres 0.07 / 0.21 / 0.32 ms (from host memory 0.08 / 0.37 / 0.81), ptmi_set_bvh_spheres 0.19 / 1.98 / 11.2 ms
 * (host 0.21 / 2.51 / 11.4), ptmi_set_scene_bvh 0.14 / 22.0 / 309 ms.  The Morton order with equal-count splits is another tree than
 * ptmi_bvh_layout's median splits: a 1080p render over it takes x 1.92 / 3.73 / 6.99 of the time over ptmi_bvh_layout's (the field is
 * flat, and the key spends 14 bits on every axis whatever its extent); over a tree REFITTED after every sphere moved by up to a tenth
 * of the field's width it takes x 1.56 / 35.8 / 216.  Refit small motions, rebuild large ones; ptmi_set_scene_bvh remains the call
 * for a static scene.
 * Under PTMI_BVH_BUILD_SPATIAL (the same tool, profiles/bvh_spatial_bench.json; another MI355X, on which bench.py implied 2.42 GHz; every
 * figure against the other builder and the host's tree in the SAME session), 1 020 / 10^5 / 10^6 spheres: the 1080p render over the
 * spatial tree takes x 1.005 / 1.021 / 0.988 of the time over ptmi_bvh_layout's (over the equal-count tree there: x 1.92 / 3.72 / 7.05);
 * the call takes 0.39 / 1.35 / 2.12 ms from device memory (from host memory 0.41 / 1.54 / 3.05), against 0.19 / 2.60 / 6.16 (0.21 / 2.79 /
 * 7.16) for the equal-count build there -- its 48 small launches and third synchronisation cost the small scene 0.2 ms, and it uploads no
 * topology.  The trees have 12 / 20 / 23 levels of inner nodes and 357 / 35 437 / 354 454 nodes; no node of them fell back to the
 * equal-count split. */
int ptmi_set_bvh_spheres(ptmi_ctx *ctx, const ptmi_sphere *spheres, int n_spheres);          /* host memory   */
int ptmi_set_bvh_spheres_device(ptmi_ctx *ctx, const ptmi_sphere *d_spheres, int n_spheres); /* device memory */

/* The host twin of ptmi_update_spheres' refit (pure host code, no device): `nodes` (n_nodes of them) and `order` as ptmi_bvh_layout or
 * ptmi_bvh_layout_morton returned them, `spheres` the moved ones.  Overwrites center, half and inv_2r of every child in place with
 * ptmi_bvh_layout's own arithmetic (csrc/ptmi_bvh_box.h); `ref` and `order` are not touched.  Unchanged spheres give ptmi_bvh_layout's
 * nodes back byte for byte, and so does moving away and back.  PTMI_EINVAL, with nothing written, for nodes and order that do not
 * belong together or non-finite sphere data. */
int ptmi_bvh_refit_layout(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int n_nodes, const int32_t *order);

/* The hierarchy ptmi_set_bvh_spheres builds, without a device (pure host code, deterministic): ptmi_bvh_layout's signature and return
 * values; it refuses what ptmi_set_bvh_spheres refuses in a sphere.  ptmi_bvh_refit_layout leaves the result byte-identical. */
int ptmi_bvh_layout_morton(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order);

/* The hierarchy ptmi_set_bvh_spheres builds under PTMI_BVH_BUILD_SPATIAL, without a device: ptmi_bvh_layout_morton's signature, return values
 * and refusals.  The leaf order ascends by (key, index) with, per axis a, q = min(16383, floor(((c[a] - lo[a]) * 16384) / den)) in f64, den the
 * LONGEST extent of the f32 box [lo, hi] of all centres (q = 0 when den is 0), interleaved as for ptmi_bvh_layout_morton.  The root is level 0;
 * a range [b, e) of more than PTMI_BVH_LEAF_MAX spheres at level L splits at the first position m whose key has the highest bit set in which
 * the range's first and last key differ, if L + 1 + levels(max(m - b, e - m)) <= PTMI_BVH_MAX_DEPTH -- levels(k) the inner levels of
 * equal-count splits over k spheres -- and at b + (e - b) / 2 otherwise or when all its keys are equal.  Nodes are numbered level by level,
 * within a level by ascending b; the boxes are ptmi_bvh_refit_layout's, which leaves the result byte-identical. */
int ptmi_bvh_layout_spatial(const ptmi_sphere *spheres, int n_spheres, ptmi_bvh_node *nodes, int node_capacity, int32_t *order);

/* The sphere hierarchy the context's BVH or mesh scene holds NOW, copied back from the device (test and diagnostic surface).  `nodes`
 * needs the scene's node count (node_capacity; PTMI_ELIMIT when too small), `order` its sphere count -- the sum of the leaves' counts
 * in `nodes` -- or NULL: the nodes alone are copied, which say how long the order is.  With both NULL nothing is copied
 * and the node count is returned.  Returns the number of nodes; PTMI_ESTATE for a linear or unset scene.  Synchronises the stream. */
int ptmi_bvh_read_layout(ptmi_ctx *ctx, ptmi_bvh_node *nodes, int node_capacity, int32_t *order);

/* screenWidth / screenHeight (src/Util.hs:186-188) as run-time values.  Allocates the
 * seven device planes the context owns (for the rows of its partition, see below) and
 * zero-fills them. */
int ptmi_resize(ptmi_ctx *ctx, int width, int height);

/* Row-stripe partition for multi-GPU runs: the image is cut into stripes of `stripe_rows`
 * rows dealt round-robin to `n_parts` contexts; this context is number `part`.  The context
 * then holds ptmi_local_rows() rows, stored contiguously in ascending global order.
 * Must be called before ptmi_resize.  Default: one part (the whole image). */
int ptmi_set_partition(ptmi_ctx *ctx, int stripe_rows, int n_parts, int part);
int ptmi_local_rows(const ptmi_ctx *ctx);                    /* rows held, or a negative code */
int ptmi_global_row(const ptmi_ctx *ctx, int local_row);     /* image row of a held row       */

/* Use caller-owned DEVICE planes (e.g. torch tensors) of ptmi_local_rows() x width elements
 * instead of the context's own; pass all NULL to return to the owned planes.  A plane needs 4-byte alignment only (16-byte aligned
 * planes let ptmi_present move four pixels per lane), and the seven may lie anywhere relative to each other: in any order, at any
 * distance, in one allocation or seven.  Nothing is written outside the ptmi_local_rows() x width elements of each.  Some NULL and some
 * not is PTMI_EINVAL and leaves the binding as it was; before ptmi_resize the call is PTMI_ESTATE.  ptmi_resize DROPS a binding:
 * afterwards the context renders into fresh owned planes, zeroed, and the caller's planes are not written again until they are bound
 * again.  Unbinding leaves the owned planes as they were when the caller's were bound: nothing is copied either way. */
int ptmi_bind_planes(ptmi_ctx *ctx, float *r, float *g, float *b,
                     uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr);
/* The device addresses of the seven planes the context currently renders into (its own or the bound ones), for
 * interop: a collective, a graphics-API import, another kernel.  Any pointer argument may be NULL. */
int ptmi_get_planes(ptmi_ctx *ctx, float **r, float **g, float **b,
                    uint32_t **sa, uint32_t **sb, uint32_t **sc, uint32_t **sctr);
/* Launch on this HIP stream (a hipStream_t cast to void*; NULL = the context's own). */
int ptmi_set_stream(ptmi_ctx *ctx, void *hip_stream);
/* Record HIP events around every ptmi_render on the launch stream (ptmi_stats.last_render_ms). */
int ptmi_set_timing(ptmi_ctx *ctx, int enabled);
/* Kernel variant selection for measurements: 0 = default.  See DESIGN.md "kernel variants". */
int ptmi_set_variant(ptmi_ctx *ctx, int variant);

/* Options.  1-5 and 8-13 concern `render Streams` (src/Scene/Trace.hs:141-191) and never change `render Inline`; 6 is a
 * scheduling knob of the per-pixel kernels that changes no result; 7 is a labelled measurement mode of `render Inline`. */
enum {
    /* Which seed a pixel carries out of `combine` (Trace.hs:179-184): the combination function keeps the seed of its
     * FIRST argument, and which of (new value, accumulator element) `permute` hands it first is backend behaviour
     * (assumption A5).  In the reference a pixel receives at most ONE result per traceStep
     * (numNewRays is 0 or 1, Trace.hs:329-331), so either reading is deterministic there.
     *   PTMI_SEED_FROM_RESULT       `f new old`, the order Accelerate's interpreter and LLVM code generators apply the
     *                               function in: every hit replaces the pixel's seed by the seed its ray carried into the
     *                               hit (computeResult, Trace.hs:317-321); updateSeed advances the survivor.  Refused for
     *                               scenes with GLASS: several results per pixel and step race for the seed there.
     *   PTMI_SEED_KEEP_ACCUMULATOR  `f old new`: the pixel keeps its seed through the sample; updateSeed advances it one draw.
     *   PTMI_SEED_AUTO (default)    FROM_RESULT -- the likelier reading -- for scenes in which no primitive splits rays (every
     *                               scene the reference can express); KEEP_ACCUMULATOR for scenes with the build-defined
     *                               GLASS, where the reference defines nothing. */
    PTMI_OPT_STREAMS_SEED_RULE = 1,
    /* Safety cap on the traceSteps of one ray lineage (children inherit their ancestors' count).  The reference has NO
     * bound (notFinished never stops a non-empty stream, Trace.hs:166-170); the default, 65536, only guarantees
     * termination, for both forms.  Rays it cuts are counted in ptmi_stats.stream_rays_truncated. */
    PTMI_OPT_STREAM_STEP_CAP = 2,
    /* Stream form only: how many rays per pixel the overflow streams hold to begin with (default 4).  (Children wait in their wave's ring in
     * LDS, then in its spill queue; the overflow streams are the last resort and practically unused: ptmi_stats.stream_rays_overflowed.)
     * The reference's vectors grow as needed (expand, Trace.hs:284-293), and since 0.5 so do these: a call that WOULD drop children puts the
     * colour planes back (they are copied aside before the launch), doubles the streams and runs again, up to 64 rays per pixel or what the
     * device's memory allows; only beyond that are children dropped and counted in ptmi_stats.stream_rays_dropped.  ptmi_get_option returns
     * the capacity in force (what the context has grown to); setting the option starts over from the value given. */
    PTMI_OPT_STREAM_CAPACITY = 3,
    /* PTMI_FORM_PIXEL: the per-pixel kernels (one lane walks its pixel's rays; with GLASS: its ray trees) -- deterministic, bit-exact against the
     * oracle also with GLASS (a colour word has one adder).
     * PTMI_FORM_STREAM: the stream ("wavefront") form -- the start hits of the pixels as a compacted list, persistent waves whose
     * lanes take items from it by ballot + prefix, refraction children compacted into a ring per wave; ONE launch per call.  With GLASS a
     * pixel's contributions are added through float atomics in no defined order (as Accelerate's permute): the same additions in another
     * association -- colours agree with the per-pixel kernels to ~1e-4 relative (1.4e-4 seen at 256 spp), the RNG planes exactly.
     * PTMI_FORM_AUTO (default): PIXEL -- except for a scene with GLASS on a PARTITIONED context (ptmi_set_partition with more than one part:
     * one rank of a multi-GPU job) at 256 samples per call or more, where it is STREAM: there the job is as fast as its slowest part, and the
     * stream form is 5 % faster on that part and evens the parts out (BASELINE configs[4]: 29.1 against 30.7 ms on the bounding part, imbalance
     * 1.02 against 1.03-1.14; at 1080p / 64 spp on one GPU it is 1 % slower, so nothing changes there).  A caller who wants the tree walk's
     * bit-exactness on such a part sets PTMI_FORM_PIXEL. */
    PTMI_OPT_STREAMS_FORM = 4,
    /* Stream form only: how many samples of a pixel make one item.  0 (default) = automatic: without GLASS a pixel's whole sample
     * chain stays in one lane, in order (bit-identical to the per-pixel kernels; few long items are cut into ORDERED passes, still
     * bit-identical); with GLASS, where the order of a pixel's additions is undefined anyway, items of a few dozen samples run in
     * whatever lanes take them.  k > 0: items of k samples -- under PTMI_SEED_FROM_RESULT (a pixel's samples are one serial chain)
     * as ordered passes, bit-identical; under PTMI_SEED_KEEP_ACCUMULATOR as unordered items: colours then agree to rounding only
     * (Accelerate's `permute` does not define the order either); the RNG planes stay exact.  A launch holds at most 64 passes: where
     * n_spp / k exceeds that, the samples are split evenly into 64 (ordered passes) or k is raised to n_spp / 64 (unordered items); with
     * PTMI_OPT_STREAM_GRADED (the default) k is the LARGEST item of the unordered form -- the last items of a launch are shorter. */
    PTMI_OPT_STREAM_BATCH = 5,
    /* The per-pixel kernels of both algorithms, a scheduling knob that changes no result: a launch of few pixels and
     * many samples (one part of a multi-GPU image) is cut into this many chained copies of the tile grid, each rendering
     * a slice of the samples, so that the end of the launch does not run on a partly empty chip.
     * 0 (default) = automatic, 1 = off, k = k copies. */
    PTMI_OPT_SPP_CHUNKS = 6,
    /* A MEASUREMENT mode of `render Inline`, never the default: PTMI_ARITH_CONTRACTED runs the same kernel compiled with
     * a * b + c contracted into fused multiply-adds (dot and cross products, the rotation, the quaternion) -- what a compiler
     * with -ffp-contract=fast, or Accelerate's fast-math LLVM backends, may do to the reference's source.  Its planes are NOT
     * the oracle's (the RNG planes still are: integer arithmetic); DESIGN.md reports how far they are and what the literal
     * reading -- every operation rounded on its own, PTMI_ARITH_EXACT -- costs.  Variants and Streams ignore it. */
    PTMI_OPT_ARITHMETIC = 7,
    /* 8-13: scheduling knobs of the stream form of Streams.  None changes a ray, a seed or (without GLASS) a bit of the planes.
     *
     * PTMI_OPT_STREAM_TAIL: scenes without GLASS, one-pass launches: the cheapest quads of the dispatch order -- the cheapest classes
     * that together hold at most this many THOUSANDTHS of the recorded cost -- are rendered by the per-pixel chain kernel on a
     * low-priority stream beside the persistent launch, whose waves' slots it fills as they end.  -1 (default) = automatic (150, or 400
     * where a lane sees fewer than four pixels), 0 = no tail. */
    PTMI_OPT_STREAM_TAIL = 8,
    /* PTMI_OPT_ORDERED_PASSES: scenes without GLASS: a pixel's samples cut into this many ORDERED passes inside the one launch; the pixel's
     * seven words are handed from the lane that rendered pass p to whichever lane -- of any wave, on any XCD -- takes pass p + 1
     * (PTMI_OPT_PASS_HANDOFF says how).  0 (default) = automatic: passes only for parts of an image at >= 256 spp, where a lane sees fewer
     * than three pixels and they are worth 5-8 % -- and only with the FENCED hand-off; 1 = OFF: one pass per launch, no hand-off between
     * waves at all; k in [2, 64] = k passes.  1 also overrides PTMI_OPT_STREAM_BATCH for scenes without GLASS.  (Until 0.4 the environment
     * variables PTMI_ORDERED_PASSES / PTMI_STREAM_TAIL overrode these two options at creation; nothing is read from the environment any more.) */
    PTMI_OPT_ORDERED_PASSES = 9,
    /* PTMI_OPT_GLASS_BATCH: scenes with GLASS: a GLASS hit waits in its lane until this many lanes of its wave hold one (or the wave has
     * nothing else to shade or trace), so that the refraction block runs for that many lanes at a time.  0 (default) = automatic,
     * 1 = off, k in [2, 64]. */
    PTMI_OPT_GLASS_BATCH = 10,
    /* PTMI_OPT_STREAM_GRADED: scenes with GLASS (or unordered items): 1 (default) = a pixel's samples are cut into GRADED passes -- long
     * items first, short ones (4 samples where the long ones hold 16 or more) last (ptmi_stream_schedule) -- so that the launch does not end with long items in few lanes;
     * 0 = uniform passes (round 3). */
    PTMI_OPT_STREAM_GRADED = 11,
    /* PTMI_OPT_SNAPSHOT_BUDGET_MB: the stream form's split kernel starts every pass of every start hit from a 16-byte seed snapshot
     * (passes x record slots x 16 bytes of device memory: 66 MB per pass at 1080p).  This caps that block: where the schedule's passes
     * would need more, its LAST passes are merged (longer items at the end of the launch; no seed and no ray changes), and a call whose
     * single pass still does not fit fails with PTMI_ELIMIT.  0 (default) = an eighth of the device's memory; otherwise megabytes
     * in [1, 2^20]. */
    PTMI_OPT_SNAPSHOT_BUDGET_MB = 12,
    /* PTMI_OPT_STREAM_PASS_GROUPS: in which order the split kernel hands out its items.  Pass by pass -- every region of the start-hit list in pass
     * 0, then every region in pass 1 ... -- a region's 64-byte records and the colour lines of its pixels come from HBM once per pass.  In GROUPS of
     * consecutive passes, each group region by region (region r in every pass of the group, then region r + 1), the items of a start hit that belong
     * to one group are taken within microseconds of each other from one ticket queue, by waves behind one L2, and only the first of them reads HBM.
     * Changes no ray and no seed, only which lane renders which item when.  0 (default) = automatic: a group is a run of passes of EQUAL size (16,
     * 16, 16 | 8 | 4, 4 at 1080p / 64 spp) -- the grading of the passes, which keeps the end of the launch short, is then untouched; 1 = every pass on
     * its own (round 4); k in [2, 64] = the LAST k passes as one group; 100 + g (g in [2, 64]) = groups of g passes all the way.
     * ptmi_stream_tickets is the order as a pure function. */
    PTMI_OPT_STREAM_PASS_GROUPS = 13,
    /* PTMI_OPT_CHAIN_SLOTS: how many states of the chained closure (ptmi_render1_chained below) may stay on the DEVICE at a time; the oldest one
     * beyond that moves to host memory the library owns (nothing is lost; ptmi_chain_fetch serves it from there).  0 (default) = automatic: what
     * a sixteenth of the device's memory holds, at least 3, at most 64; otherwise k in [2, 4096]. */
    PTMI_OPT_CHAIN_SLOTS = 14,
    /* PTMI_OPT_PASS_HANDOFF: how ordered passes (PTMI_OPT_ORDERED_PASSES) hand a pixel's words from wave to wave.
     * PTMI_HANDOFF_FENCED (default): what the HSA memory model promises -- the storing wave's vmcnt(0), an agent-scope RELEASE, the region's
     * counter; the taking wave's poll, an agent-scope ACQUIRE, its loads -- paid once per (region, pass), not per item: all items of a region's
     * pass run in the one wave that drew its ticket, and the lane that ends the last of them releases for all.
     * PTMI_HANDOFF_FENCE_FREE: rounds 3-5's form -- write-through (sc1) stores, a counter that moves after the storing wave's vmcnt(0), sc1
     * loads after the poll, NO fence: the "valid form" of MI355X_MICROARCH.md, MEASURED valid on gfx950 (5 billion hand-offs compared bit for
     * bit, profiles/r05_soak_ordered_passes.json) -- not a promise of the memory model.  Never chosen automatically: with this value
     * PTMI_OPT_ORDERED_PASSES = 0 means one pass. */
    PTMI_OPT_PASS_HANDOFF = 15,
    /* (16 is unused.)  PTMI_OPT_BVH_DEVICE_BUILD: which sphere hierarchy LATER calls of ptmi_set_bvh_spheres[_device] and
     * ptmi_group_set_bvh_spheres build, on BVH and on mesh scenes; the scene held is not touched, and ptmi_set_scene_bvh, ptmi_set_scene_mesh,
     * ptmi_update_spheres and the mesh triangle calls do not look at it.
     * PTMI_BVH_BUILD_EQUAL_COUNT (default): keys scaled per axis, every range split at its middle -- ptmi_bvh_layout_morton's tree.
     * PTMI_BVH_BUILD_SPATIAL: keys in CUBIC cells (one scale, that of the longest axis of the centres' box), every range split where the
     * highest differing key bit changes, within PTMI_BVH_MAX_DEPTH (a split that would leave no room for the larger side falls back to the
     * middle) -- ptmi_bvh_layout_spatial's tree, which renders about as fast as ptmi_bvh_layout's (see ptmi_set_bvh_spheres). */
    PTMI_OPT_BVH_DEVICE_BUILD = 17
};
enum { PTMI_BVH_BUILD_EQUAL_COUNT = 0, PTMI_BVH_BUILD_SPATIAL = 1 };
enum { PTMI_HANDOFF_FENCED = 0, PTMI_HANDOFF_FENCE_FREE = 1 };
enum { PTMI_ARITH_EXACT = 0, PTMI_ARITH_CONTRACTED = 1 };
enum { PTMI_SEED_KEEP_ACCUMULATOR = 0, PTMI_SEED_FROM_RESULT = 1, PTMI_SEED_AUTO = 2 };
enum { PTMI_FORM_AUTO = 0, PTMI_FORM_STREAM = 1, PTMI_FORM_PIXEL = 2 };
int ptmi_set_option(ptmi_ctx *ctx, int option, int64_t value);
/* The passes the stream form's split kernel (GLASS, or PTMI_OPT_STREAM_BATCH under PTMI_SEED_KEEP_ACCUMULATOR) cuts n_spp samples into
 * for n_pixels held pixels on `lanes` persistent lanes (64 x 4 x 6 x compute units): pass p renders samples [first[p], first[p + 1]).
 * batch = PTMI_OPT_STREAM_BATCH, graded = PTMI_OPT_STREAM_GRADED.  Pure host arithmetic (no device needed).  Returns the number of
 * passes (first[] receives passes + 1 entries), PTMI_ELIMIT if `capacity` entries do not hold them (65 always do). */
int ptmi_stream_schedule(int n_spp, uint64_t n_pixels, uint64_t lanes, int batch, int graded, int32_t *first, int capacity);
/* The schedule of the cost-ordered dispatch, host arithmetic: given the launches made so far with one (camera, scene,
 * shape, limit, algorithm), does the next launch rebuild the order from the recorded costs (before launch 1, 2, 4, 8, ...; never once
 * the recording limit -- 2^20 launches, 2^11 for the stream form -- is reached) and does it record its costs (only if the launch after it
 * rebuilds: launch 0, 1, 3, 7, 15, ...)?  Returns the state after it. */
int ptmi_order_schedule(int launches, int stream_form, int *rebuild, int *record);
/* The order in which ONE of the eight ticket queues of the split kernel hands out its passes x queue_regions items under
 * PTMI_OPT_STREAM_PASS_GROUPS = option, for the schedule first[0 .. passes] of ptmi_stream_schedule: ticket j is (pass_out[j], region_out[j]),
 * region = the region's index within the queue.  Every (pass, region) pair appears exactly once.  Pure host arithmetic.  Returns the number of
 * tickets, PTMI_ELIMIT if `capacity` entries do not hold them. */
int ptmi_stream_tickets(int option, const int32_t *first, int passes, int queue_regions, int32_t *pass_out, int32_t *region_out, int capacity);
int ptmi_get_option(ptmi_ctx *ctx, int option, int64_t *value);

/* ---- state: initialOutput / genSeeds / reseed -------------------------------- */
/* initialOutput (src/Util.hs:204-205): colour := 0, RNG := genSeeds.  genSeeds draws three
 * words per pixel from OS entropy (src/Util.hs:122-127); here they come from a counter-based
 * hash of (seed0, global pixel index) so that "the same RNG seed" is meaningful, then go
 * through createWith (3-word sfc32 seeding).  Runs on the device. */
int ptmi_init_output(ptmi_ctx *ctx, uint64_t seed0);
/* reseed (src/Util.hs:134-135): keep colour, replace every RNG state. */
int ptmi_reseed(ptmi_ctx *ctx, uint64_t seed0);
/* createWith . use (src/Util.hs:125): three host word planes -> RNG states (colour untouched). */
int ptmi_create_with(ptmi_ctx *ctx, const uint32_t *w0, const uint32_t *w1, const uint32_t *w2);
/* Host <-> device copies of the held rows (synchronous). NULL plane pointers are skipped. */
int ptmi_upload_state(ptmi_ctx *ctx, const float *r, const float *g, const float *b,
                      const uint32_t *sa, const uint32_t *sb, const uint32_t *sc, const uint32_t *sctr);
int ptmi_download_state(ptmi_ctx *ctx, float *r, float *g, float *b,
                        uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr);
int ptmi_download_color(ptmi_ctx *ctx, float *r, float *g, float *b);   /* what graphicsLoop reads, Main.hs:350 */

/* ---- the hot path ------------------------------------------------------------- */
/* Resident form: equivalent to n_spp successive applications of
 *     render algorithm screenPixels camera            (src/Scene/Trace.hs:135-200)
 * to the planes held by the context.  `bounce_limit` is the `15` of Trace.hs:200 /
 * maxIterations (:80-81) made a parameter; PTMI_STREAMS IGNORES it, as the reference's Streams does (a non-empty
 * stream is never stopped by the iteration count, Trace.hs:166-170) -- ptmi_stats.nominal_bounces is therefore 0 for
 * Streams launches and live_bounces counts the child rays they emitted.  Asynchronous on the launch stream. */
int ptmi_render(ptmi_ctx *ctx, const ptmi_camera *camera, int algorithm,
                int bounce_limit, int n_spp);
int ptmi_synchronize(ptmi_ctx *ctx);
/* 1 if ptmi_render with `algorithm` would wait for device work before it returns under the context's present scene and options
 * (the stream form of Streams with GLASS, or with PTMI_OPT_STREAM_BATCH, reads its overflow counters back), 0 if it only enqueues. */
int ptmi_render_blocks(ptmi_ctx *ctx, int algorithm);

/* Compatibility form = exactly one call of the closure built by compileFor: host planes in,
 * host planes out, one sample.  screen_x / screen_y are the two Int planes of the
 * Matrix (V2 Int) argument (src/Util.hs:209-210) or NULL for the implicit x = column,
 * y = row.  Pointers are borrowed for the duration of the call; in and out may alias.
 * Ignores any partition: the whole width x height image is rendered. */
int ptmi_render1(ptmi_ctx *ctx, const ptmi_camera *camera, int algorithm, int bounce_limit,
                 int width, int height,
                 const int64_t *screen_x, const int64_t *screen_y,
                 const float *r_in, const float *g_in, const float *b_in,
                 const uint32_t *sa_in, const uint32_t *sb_in, const uint32_t *sc_in, const uint32_t *sctr_in,
                 float *r_out, float *g_out, float *b_out,
                 uint32_t *sa_out, uint32_t *sb_out, uint32_t *sc_out, uint32_t *sctr_out);

/* ---- the closure, chained: device residency behind compileFor's pure type ------------------------------------------------
 * `dewit = runN (render config) screenPixels` (app/Main.hs:190) is a pure function of arrays, and on the reference's own GPU backend
 * those arrays LIVE ON THE DEVICE: runN leaves its result there and copies it to the host lazily, when somebody reads it
 * (graphicsLoop, app/Main.hs:350), and an argument that is a previous result is found on the device again and not uploaded.
 * ptmi_render1 above moves all seven planes both ways on every call (1.1 ms per sample at 800x600 around a 0.03-ms kernel);
 * these entry points give the closure runN's behaviour.  A STATE is one RenderResult (seven planes, width x height) held by the
 * context under a TOKEN (never 0, never reused, meaningless to other contexts).  To the caller a state is an immutable value:
 *   - ptmi_render1_chained(token_in) renders ONE sample from the state token_in names into a NEW state and returns its token; the
 *     input state stands as it was, for ptmi_chain_fetch or for another call (rendering twice from one token gives the same planes
 *     twice -- the closure is a function).  Nothing crosses PCIe; the call only enqueues.
 *   - if token_in names no state the context holds (0; a released token; a RenderResult that came from elsewhere), the seven host
 *     planes r_in .. sctr_in are uploaded instead -- ptmi_render1's copy path; if they are NULL too: PTMI_ESTALE.
 *   - planes_out: each may be NULL; the ones given are downloaded at once (the call then waits for the render).  A lazy consumer
 *     passes none and calls ptmi_chain_fetch when somebody reads a plane: colour for graphicsLoop, all seven on demand.
 *   - a state is held until ptmi_chain_release(token) (a Haskell finalizer, a C++ destructor), or until a call CONSUMES it
 *     (PTMI_CHAIN_CONSUME: the caller gives up token_in with the call; the sample is then rendered in place, without the
 *     device-to-device copy that otherwise keeps the input intact -- the cost of a resident ptmi_render; should the call then fail, the
 *     input is gone with it).  At most
 *     PTMI_OPT_CHAIN_SLOTS states stay on the device; older ones move to host memory the library owns and are served from there.
 * Any thread; calls are serialised by the context's mutex like all others.  The resident planes of ptmi_resize / ptmi_render and
 * their partition are a separate matter and untouched. */
enum { PTMI_CHAIN_CONSUME = 1 };
int ptmi_render1_chained(ptmi_ctx *ctx, const ptmi_camera *camera, int algorithm, int bounce_limit, int width, int height,
                         uint64_t token_in, int flags,
                         const float *r_in, const float *g_in, const float *b_in,
                         const uint32_t *sa_in, const uint32_t *sb_in, const uint32_t *sc_in, const uint32_t *sctr_in,
                         uint64_t *token_out,
                         float *r_out, float *g_out, float *b_out,
                         uint32_t *sa_out, uint32_t *sb_out, uint32_t *sc_out, uint32_t *sctr_out);
/* run <$> initialOutput (src/Util.hs:204-205; app/Main.hs:155, :306) as a state: colour 0, RNG from seed0 (ptmi_init_output's seeding). */
int ptmi_chain_init_output(ptmi_ctx *ctx, int width, int height, uint64_t seed0, uint64_t *token_out);
/* run <$> reseed acc (src/Util.hs:134-135; app/Main.hs:231): a NEW state with token_in's colour and fresh RNG states from seed0.  If
 * token_in is not held the three colour planes r_in, g_in, b_in (host) are uploaded instead.  flags: PTMI_CHAIN_CONSUME as above. */
int ptmi_chain_reseed(ptmi_ctx *ctx, uint64_t seed0, int width, int height, uint64_t token_in, int flags,
                      const float *r_in, const float *g_in, const float *b_in, uint64_t *token_out);
/* The planes of a held state into host memory; NULL pointers are skipped.  Waits for the renders that produce the state. */
int ptmi_chain_fetch(ptmi_ctx *ctx, uint64_t token, float *r, float *g, float *b,
                     uint32_t *sa, uint32_t *sb, uint32_t *sc, uint32_t *sctr);
/* The caller will not name this token again.  Releasing a token that is not held (already released or consumed) is PTMI_OK. */
int ptmi_chain_release(ptmi_ctx *ctx, uint64_t token);
typedef struct ptmi_chain_stats {
    uint32_t states_on_device, states_on_host;    /* held now */
    uint32_t device_slots;                         /* PTMI_OPT_CHAIN_SLOTS in force */
    uint32_t width, height;                        /* of the newest state (0 when none is held) */
    uint64_t renders_chained;                      /* ptmi_render1_chained / ptmi_chain_reseed calls that found their input on the device ... */
    uint64_t renders_in_place;                     /* ... of which PTMI_CHAIN_CONSUME spared the copy                                         */
    uint64_t renders_uploaded;                     /* calls that took the copy path (host planes in)                                           */
    uint64_t evictions;                            /* states moved to host memory to make room                                                 */
    uint64_t fetches;                              /* ptmi_chain_fetch calls and planes_out downloads                                          */
} ptmi_chain_stats;
int ptmi_chain_info(ptmi_ctx *ctx, ptmi_chain_stats *out);

/* ---- present (what graphicsLoop + fs.glsl do with the result) ------------------- */
/* graphicsLoop interleaves the three colour planes (`V.zipWith3 V3 r g b`, app/Main.hs:351), uploads them
 * as an RGB32F texture (:383-393) and the fragment shader shows `texture.rgb / u_iterations`
 * (app/assets/fs.glsl:12) into an 8-bit framebuffer.  This does the same on the device for the held rows:
 *   rgb32f_out : [rows][W][3] float, colour / float(iterations)            (may be NULL)
 *   rgba8_out  : [rows][W][4] bytes, round(clamp(colour / iterations, 0, 1) * 255), alpha 255   (may be NULL)
 * The text overlay of the iteration counter (fs.glsl:15) is UI and not reproduced. */
int ptmi_present(ptmi_ctx *ctx, int iterations, float *rgb32f_out, uint8_t *rgba8_out);

/* The three colour planes of the held rows, copied device-to-device into ONE contiguous buffer [3][rows][W] on the
 * context's device, ordered behind the renders already issued; the copy runs on `hip_stream` (a hipStream_t cast to
 * void*; NULL = the context's launch stream), so a consumer (a collective, a display interop) can take it from there
 * while the next render runs.  Asynchronous. */
int ptmi_snapshot_color(ptmi_ctx *ctx, float *dst_device, void *hip_stream);

int ptmi_get_stats(ptmi_ctx *ctx, ptmi_stats *out);   /* synchronises the launch stream */
int ptmi_reset_stats(ptmi_ctx *ctx);
/* Diagnostics: the raw device counters (hand-out counter in [0]; the diagnostic builds of the kernels --
 * -DPTMI_PHASE_STATS and the others listed in csrc/ptmi_diag.h -- add their statistics, see tools/phase_stats.py).
 * ptmi_debug_counters writes the first 64 words (its contract since 0.3; 0.4 wrote 256 into the same argument and overran a
 * caller built against 0.3); ptmi_debug_counters_n writes min(capacity, 256) words and returns how many, or a negative code.
 * A caller built against 0.4 that passes a 256-word buffer to ptmi_debug_counters gets PTMI_OK and words 64 to 255 LEFT AS THEY WERE:
 * it must move to ptmi_debug_counters_n to see the diagnostic builds' statistics.  Both synchronise the launch stream. */
int ptmi_debug_counters(ptmi_ctx *ctx, uint32_t out[64]);
int ptmi_debug_counters_n(ptmi_ctx *ctx, uint32_t *out, int capacity);

/* ---- groups: the GPUs of one node behind ONE host process ------------------------ */
/* The reference's host is a single process holding one compiled function (app/Main.hs:188-191); a group lets that
 * process use several GPUs: the image is cut into stripes of `stripe_rows` rows (0 = 8) dealt round-robin to the
 * devices (ptmi_set_partition), every member renders its rows without any exchange (seeds come from the global pixel
 * index: the stitched planes equal the single-device image bit for bit), and the one exchange is the read-out of the
 * colour planes -- to host planes for graphicsLoop (app/Main.hs:346-351), or to a root device over RCCL / xGMI.
 * (SURVEY.md 8b proposed ptmi_create(out, device_first, n_devices); a group of contexts keeps ptmi_create unchanged.) */
typedef struct ptmi_group ptmi_group;
int         ptmi_group_create(ptmi_group **out, const int *devices, int n_devices, int stripe_rows);
void        ptmi_group_destroy(ptmi_group *group);
int         ptmi_group_size(const ptmi_group *group);
ptmi_ctx   *ptmi_group_member(ptmi_group *group, int i);        /* member i's context (options, statistics, planes) */
const char *ptmi_group_last_error(const ptmi_group *group);      /* per thread, as ptmi_last_error */
int ptmi_group_set_scene(ptmi_group *group, const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes);
int ptmi_group_set_scene_bvh(ptmi_group *group, const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes);   /* ptmi_set_scene_bvh on every member */
int ptmi_group_set_scene_mesh(ptmi_group *group, const ptmi_sphere *spheres, int n_spheres, const ptmi_triangle *triangles, int n_triangles,
                              const ptmi_plane *planes, int n_planes);   /* ptmi_set_scene_mesh on every member */
int ptmi_group_update_mesh_vertices(ptmi_group *group, const float *vertices, int n_triangles);   /* ptmi_update_mesh_vertices on every member */
int ptmi_group_set_mesh_triangles(ptmi_group *group, const ptmi_triangle *triangles, int n_triangles);   /* ptmi_set_mesh_triangles on every member */
int ptmi_group_update_spheres(ptmi_group *group, const float *geometry, int n_spheres);   /* ptmi_update_spheres on every member */
int ptmi_group_set_bvh_spheres(ptmi_group *group, const ptmi_sphere *spheres, int n_spheres);   /* ptmi_set_bvh_spheres on every member */
int ptmi_group_resize(ptmi_group *group, int width, int height);
int ptmi_group_init_output(ptmi_group *group, uint64_t seed0);
int ptmi_group_reseed(ptmi_group *group, uint64_t seed0);
/* ptmi_set_option / ptmi_set_variant on every member (ptmi_group_member gives access to a single one). */
int ptmi_group_set_option(ptmi_group *group, int option, int64_t value);
int ptmi_group_set_variant(ptmi_group *group, int variant);
/* ptmi_render on every member; asynchronous: all devices are busy before the call returns. */
int ptmi_group_render(ptmi_group *group, const ptmi_camera *camera, int algorithm, int bounce_limit, int n_spp);
int ptmi_group_synchronize(ptmi_group *group);
/* The whole image's colour planes [height][width] into HOST planes: every member's rows come down through its own
 * copy path, all members at once, and the stripes are stitched in place.  Synchronous. */
int ptmi_group_download_color(ptmi_group *group, float *r, float *g, float *b);
/* The whole image's colour planes into DEVICE planes [height][width] on member `root`'s device: RCCL grouped
 * ncclSend / ncclRecv over xGMI (every peer has its own link to the root), then a stitch kernel.  Synchronous.  The
 * caller's current HIP device is left as it was.  (What has run: on real RCCL, one member sending to itself; with 3 and 8 members
 * sharing one device, the whole n > 1 call sequence -- every root, unequal row counts, members without rows, communicator reuse, an
 * error inside the group -- against a test-only stand-in for librccl that turns paired sends and receives into device copies
 * (tests/test_gpu_group_rccl_stub.py: the host logic).  Between PHYSICAL devices, over xGMI, it has never run: no box this build has
 * seen holds two GPUs; tests/test_group.py arms itself on the first one that does.) */
int ptmi_group_gather_color(ptmi_group *group, int root, float *r_device, float *g_device, float *b_device);
int ptmi_group_get_stats(ptmi_group *group, ptmi_stats *sum);  /* sums (maxima for the time and step fields) over the members */
/* The partition's arithmetic, usable without a device: rows part `part` holds, and the image row of one of them. */
int ptmi_partition_rows(int height, int stripe_rows, int n_parts, int part);
int ptmi_partition_global_row(int height, int stripe_rows, int n_parts, int part, int local_row);

/* ---- ray queries on the device ------------------------------------------------ */
/* The caller's own rays against the context's current scene -- linear, BVH or mesh -- without leaving the device: closest hit with its hit
 * record, and occlusion before a distance (shadow and visibility rays, range sensors).  d_rays: n x 6 floats (origin, direction), as
 * ptmi_eval_check_hit takes them, in device memory of the context's device, like every other array here; each needs 4-byte alignment only
 * (8-byte aligned rays and hit records are moved two words at a time).
 *   - ORDER AND LIFETIME.  One launch on the context's launch stream (ptmi_set_stream), and nothing else: no host synchronisation, no
 *     device allocation, no staging.  The caller orders its writes to the inputs before that stream (they are on it, or an event makes it
 *     wait), keeps every array alive until the stream has passed the call, and reads the outputs behind the stream.  A later scene call on
 *     the same context -- a move, a refit, a replacement, another scene -- is ordered behind the query: the query answers for the scene as
 *     it stood at the call, and a query enqueued after an update answers for the updated scene.
 *   - ptmi_trace_rays_device: d_t[i] and d_idx[i] are ptmi_eval_check_hit's t_out[i] and idx_out[i] for ray i, bit for bit (the same
 *     device functions): the primitive by the existing convention, spheres, then planes, then triangles; a miss is t = 0, idx = -1, so
 *     idx >= 0 says Just.  d_hit, unless NULL, receives n x 6 floats: the hit position o + d ^* t and the normal of the selected primitive
 *     as the render kernels compute them (a sphere's normalised (p - centre), a plane's stored direction, a triangle's unit normal); six
 *     zeros for a miss.
 *   - ptmi_occluded_device: d_occluded[i] = 1 if the closest hit of ray i is a Just and its t < d_t_max[i] (one binary32 compare against
 *     that same closest hit), else 0.  So a NaN or non-positive t_max gives 0, and +inf asks whether the ray hits anything at a finite t.
 *     It is computed by an any-hit walk that stops at the first primitive that decides the answer and enters no box beyond t_max; where
 *     that would not provably equal the definition -- a ray the hierarchies do not serve, a plane whose key is not finite -- the lane
 *     takes the closest-hit search and compares (csrc/ptmi_query_device.h has the argument, DESIGN.md 5.9 the measurements).
 *   - Refusals enqueue and write nothing: PTMI_ESTATE before any scene is set; PTMI_EINVAL for a negative n and for a NULL required
 *     pointer with n > 0 (d_hit may be NULL).  n == 0 is PTMI_OK and touches nothing.  The pointers are not inspected: an address that
 *     is not device memory of the context's device fails as any kernel's would.
 *   - There is no group form: a group's members are different devices and an array of rays lives on one.  Query a member
 *     (ptmi_group_member) with rays on its device. */
int ptmi_trace_rays_device(ptmi_ctx *ctx, const float *d_rays, int n, float *d_t, int32_t *d_idx, float *d_hit /* [n][6] position, normal; may be NULL */);
int ptmi_occluded_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, int32_t *d_occluded);

/* ---- ray order and ray queries through an index ------------------------------- */
/* The queries above take one lane per ray in the caller's order: a wave whose 64 rays point everywhere walks 64 paths through a hierarchy.
 * Two things serve the batches real callers send (bounce rays, shadow rays from scattered points, sensor beams), through one mechanism,
 * an index array of int32 in device memory.  The order and lifetime rules are those of the section above, for every array here, the
 * workspace included.
 *   - ptmi_ray_order_device: d_order receives a permutation of 0 .. n - 1, ascending by (key, original index).  The key is a function of
 *     the rays alone (csrc/ptmi_ray_order.h states it): 24 bits of Morton code of the origin's cell in the box of the batch's origins, then
 *     20 bits of Morton code of the direction's cell on the octahedral map -- origins major, so bounce rays group by place and a camera's
 *     rays by direction; a ray with a non-finite word or a zero direction sorts behind every other, in index order.  No scene is needed
 *     (no PTMI_ESTATE).  d_work: ptmi_ray_order_bytes(n) bytes, 8-byte aligned, scratch while the call is in flight.  Everything is
 *     enqueued on the context's stream: no host synchronisation, no allocation, no copy to the host.  Refusals enqueue and write nothing:
 *     PTMI_EINVAL for a negative n, for a NULL pointer with n > 0, for a d_work that is not 8-byte aligned and for work_bytes below
 *     ptmi_ray_order_bytes(n); PTMI_ELIMIT for n > PTMI_RAY_ORDER_MAX.  n == 0 is PTMI_OK and touches nothing.
 *   - ptmi_ray_order / ptmi_ray_order_keys: the same order, and the keys themselves (1 << 44 for a ray that is not placed), from HOST rays
 *     on the host: no context, no device.  The specification the device order is tested against.
 *   - ptmi_trace_rays_indexed_device / ptmi_occluded_indexed_device: lane k < m takes i = d_index[k]; if 0 <= i < n it answers ray i and
 *     writes the answer at position i of the outputs -- the n-sized arrays of the plain entries -- with the plain entries' words, bit for
 *     bit (the same device functions), whatever the index holds.  An entry outside [0, n) is skipped: nothing is read or written for it.
 *     A position no entry names is left untouched; one named twice is written twice with the same words.  With ptmi_ray_order_device's
 *     order as the index this is the reordered query; with a caller's list of live rays (m < n), the active-list query.  Refusals are
 *     the plain entries', and PTMI_EINVAL for a negative m or a NULL d_index with m > 0; m == 0 is PTMI_OK and touches nothing.
 *   - Ordering pays where rays diverge in a hierarchy (BVH and mesh scenes, incoherent batches) and one order serves several queries; it
 *     does not pay on a linear scene, which has no hierarchy to diverge in, on rays that are coherent already, or for a single query: the
 *     order costs about as much as a trace (DESIGN.md 5.9 has the measurements).
 *   - There is no group form, as above. */
#define PTMI_RAY_ORDER_MAX (1 << 22)   /* what the builders' sort is tested at */
size_t ptmi_ray_order_bytes(int n);    /* workspace for n rays; 0 for n <= 0 */
int ptmi_ray_order_device(ptmi_ctx *ctx, const float *d_rays, int n, int32_t *d_order, void *d_work, size_t work_bytes);
int ptmi_ray_order(const float *rays, int n, int32_t *order);
int ptmi_ray_order_keys(const float *rays, int n, uint64_t *keys);
int ptmi_trace_rays_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m,
                                   float *d_t, int32_t *d_idx, float *d_hit /* may be NULL */);
int ptmi_occluded_indexed_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m,
                                 int32_t *d_occluded);

/* ---- multi-hit: the k nearest hits along a caller's rays ----------------------- */
/* The first k hits in order, within t_max: what lies between a point and a light (a shadow ray through GLASS), every return along a
 * sensor's beam, the ordered crossings of a thickness query.  The order, lifetime and refusal rules are ptmi_trace_rays_device's: one
 * launch on the context's stream, no host wait, no allocation, no copy.  d_t and d_idx hold n x k words (row i at k i), d_count n.
 *   - QUALIFYING HITS.  For ray i with lim = d_t_max ? d_t_max[i] : +inf, H is the set of pairs (t_j, j) over ALL primitives j of the
 *     scene -- spheres, then planes, then triangles -- whose own test is a Just and whose t_j < lim, one binary32 compare.  The own tests
 *     are the closest hit's, from the same text: a sphere's distanceTo with the correctly rounded root and !(t < 0), a plane's behind the
 *     candidate test !(denom > 1e-6), the triangle test, a zero-area triangle never a Just.  Each primitive contributes at most one hit:
 *     a sphere gives its entry point only.  A NaN t fails the compare, and +inf fails it against any lim: every listed t is finite and
 *     >= 0, and a NaN or non-positive t_max gives an empty list.
 *   - THE OUTPUT.  d_count[i] = min(k, |H|); row i of d_t and d_idx holds the d_count[i] smallest elements of H ascending by (t, j),
 *     lexicographically -- at equal t the lower primitive index first, the closest hit's tie rule -- and the rest of the row the miss
 *     record, t = 0 and idx = -1.
 *   - Where no primitive's key for the ray is a NaN, column 0 at k = 1 without d_t_max is ptmi_trace_rays_device's (t, idx), and
 *     d_count > 0 at k = 1 is ptmi_occluded_device under the same t_max.
 *   - ptmi_trace_rays_multi_indexed_device: lane p < m takes i = d_index[p]; an entry outside [0, n) is skipped, the answer goes to row
 *     i with the plain entry's words, and a position no entry names is left untouched.
 *   - Refusals enqueue and write nothing: PTMI_ESTATE before a scene is set; PTMI_EINVAL for a negative n or m, for k < 1 and for a NULL
 *     required pointer with work to do (d_t_max may be NULL); PTMI_ELIMIT for k > PTMI_MULTI_HIT_MAX.  n == 0 or m == 0 is PTMI_OK and
 *     touches nothing.  The context's planes, statistics and dispatch order are left alone.
 *   - A hierarchy's walk is bounded by the k-th key the lane holds, so k = 1 costs about a closest hit and a larger k walks further;
 *     without t_max and with k above the hits there are, the walk visits everything the ray's boxes touch (csrc/ptmi_multi_hit_device.h
 *     has the argument, DESIGN.md 5.9 the measurements).
 *   - There is no group form, as above. */
#define PTMI_MULTI_HIT_MAX 16
int ptmi_trace_rays_multi_device(ptmi_ctx *ctx, const float *d_rays /* [n][6] */, const float *d_t_max /* [n], or NULL: +inf for every ray */,
                                 int n, int k, float *d_t /* [n][k] */, int32_t *d_idx /* [n][k] */, int32_t *d_count /* [n] */);
int ptmi_trace_rays_multi_indexed_device(ptmi_ctx *ctx, const float *d_rays, const float *d_t_max, int n, const int32_t *d_index, int m,
                                         int k, float *d_t, int32_t *d_idx, int32_t *d_count);

/* ---- the nearest-primitive query: the primitive nearest to a caller's points ---- */
/* The companion of the ray queries: which primitive is nearest to this point, how far away is it, and where on it is the nearest location --
 * the clearance of a sensor from the scene, a distance field sampled into a grid, points snapped to surfaces, "is anything within r of
 * here".  d_points holds n x 3 words, d_r_max n (or NULL), d_dist and d_idx n, d_point n x 3 (or NULL: no locations wanted).  The order,
 * lifetime and refusal rules are ptmi_trace_rays_multi_device's: one launch on the context's stream, no host wait, no allocation, no
 * copy; 4-byte alignment suffices for every array.
 *   - THE ANSWER.  For point i with lim = d_r_max ? d_r_max[i] : +inf, every primitive j of the current scene -- linear, BVH or mesh;
 *     spheres, then planes, then triangles -- has a signed distance s_j and the key |s_j|, and the answer is the minimum of (key, j),
 *     lexicographically (at equal keys the lower index), over the primitives with key < lim, one binary32 compare.  A NaN or +inf key
 *     never qualifies; a NaN or non-positive r_max gives a miss.  d_dist[i] = s_j, NEGATIVE BEHIND THE SURFACE (inside a sphere, behind a
 *     plane's or a triangle's front), d_idx[i] = j and d_point[i] the nearest location on primitive j.  A miss is dist 0, idx -1,
 *     location (0, 0, 0).
 *   - THE DISTANCES are binary32, every operation rounded on its own, on coordinates RELATIVE TO THE POINT, so that their error is a
 *     small multiple of 2^-24 times the distance to the primitive's farthest point, wherever the scene lies (csrc/ptmi_nearest.h, the
 *     one definition of device and host).  A sphere (c, r): |p - c| - r, the location c + (p - c) r / |p - c|, at the centre
 *     (cx + r, cy, cz).  A plane: dot(p - pos, dir) / |dir|, dir as stored and divided by its length here; a zero or non-finite
 *     direction is no candidate.  A triangle: the distance to its plane where p's foot on the plane lies inside or on an edge, otherwise
 *     the least distance to its three edges; its normal is formed from the relative coordinates with compensated products, so a needle
 *     or a sliver is served as accurately as any other shape; negative when p is behind the front.  A triangle of zero area is no
 *     candidate, as for rays.
 *   - ptmi_nearest_indexed_device: lane k < m takes i = d_index[k]; an entry outside [0, n) is skipped, the answer goes to position i,
 *     and a position no entry names is left untouched.
 *   - Refusals enqueue and write nothing: PTMI_ESTATE before a scene is set; PTMI_EINVAL for a negative n or m and for a NULL required
 *     pointer with work to do (d_r_max and d_point may be NULL).  n == 0 or m == 0 is PTMI_OK and touches nothing.  The context's
 *     planes, statistics and dispatch order are left alone.
 *   - A hierarchy's walk is bounded by the best key so far, which starts at r_max: a small r_max visits little, and a point far from
 *     everything without one visits much (csrc/ptmi_nearest_device.h has the argument that the winner is never pruned).  A point with a
 *     non-finite word, or farther than 2^40 from a hierarchy's box, enumerates every primitive.
 *   - ptmi_nearest is the HOST TWIN: no context, no device; the same answers by enumeration, from the same functions -- the definition
 *     the device entries are held to.  r_max and point may be NULL.  With triangles it refuses what ptmi_set_scene_mesh refuses in the
 *     scene data, by that call's own checks: counts beyond PTMI_MAX_BVH_* and PTMI_MAX_MESH_TRIANGLES (PTMI_ELIMIT), an unknown brdf_tag,
 *     non-finite sphere or triangle geometry, a non-finite triangle material (PTMI_EINVAL); without triangles it takes the data as a
 *     linear scene does.  An empty scene, a negative count or a NULL required pointer with work to do is PTMI_EINVAL.
 *   - There is no group form, as above. */
int ptmi_nearest_device(ptmi_ctx *ctx, const float *d_points /* [n][3] */, const float *d_r_max /* [n], or NULL: +inf for every point */, int n,
                        float *d_dist /* [n] */, int32_t *d_idx /* [n] */, float *d_point /* [n][3], may be NULL */);
int ptmi_nearest_indexed_device(ptmi_ctx *ctx, const float *d_points, const float *d_r_max, int n, const int32_t *d_index, int m,
                                float *d_dist, int32_t *d_idx, float *d_point);
int ptmi_nearest(const ptmi_sphere *spheres, int n_spheres, const ptmi_plane *planes, int n_planes, const ptmi_triangle *triangles, int n_triangles,
                 const float *points, const float *r_max, int n, float *dist, int32_t *idx, float *point);

/* ---- paths along a caller's rays ---------------------------------------------- */
/* The third question about a caller's own device-resident rays, the one only a camera could ask so far: what light arrives along this ray
 * (traceInline, src/Scene/Trace.hs:344-383).  It serves cameras ptmi_camera cannot describe (fisheye, orthographic, thin lens), jittered
 * primaries, light probes, sensor positions and paths continued from a caller's own first bounce.  d_rays is the ray queries' array;
 * d_color holds n x 3 floats (r, g, b of ray i at 3 i) and d_seed n x 4 words (the SFC32 state a, b, c, counter of ray i at 4 i), both
 * read and written.  The order, lifetime and alignment rules are those of "ray queries on the device": one launch on the context's
 * launch stream, no host synchronisation, no device allocation, no copy; a later scene call is ordered behind it; 4-byte alignment
 * suffices for every array (8-byte aligned rays and 16-byte aligned seeds are moved in wider pieces).
 *   - ptmi_trace_paths_device does for ray i what ptmi_render(PTMI_INLINE) does for a pixel, with the render kernels' own arithmetic:
 *         repeat n_spp times:  (new, seed') = traceInline bounce_limit scene ray_i seed_i;  color_i = new + color_i;  seed_i = seed'
 *     so the primary rays of a ptmi_camera, ptmi_path_seeds_device's seeds and a zero colour give ptmi_init_output + ptmi_render's seven
 *     planes bit for bit, and one call of n_spp samples equals n_spp calls of one.  The ray is taken as given, with a direction of any
 *     length; a ray with a non-finite word goes wherever checkHit and the shade take it.  bounce_limit <= 0 with n_spp > 0 gives
 *     color_i = 0 + color_i and leaves the seed as it was; n_spp <= 0 or n == 0 is PTMI_OK and touches nothing.  The scene is the context's
 *     current one of any kind: linear, BVH or mesh.  The context's state planes, partition, camera and statistics are not touched.
 *   - ptmi_path_seeds_device fills d_seed[i] with the state ptmi_init_output(seed0) gives pixel first_index + i of an unpartitioned image
 *     (genSeeds, src/Util.hs:122-135).  It needs no scene (no PTMI_ESTATE); n == 0 is PTMI_OK.
 *   - ptmi_trace_paths_indexed_device follows the indexed queries' contract: lane k < m takes i = d_index[k]; an entry outside [0, n) is
 *     skipped, nothing is read or written for it; a position no entry names is left untouched; m == 0 is PTMI_OK.  Colour and seed are
 *     read, modified and written, so the index must name a ray AT MOST ONCE: a ray named twice is a race between two lanes, and its
 *     colour and seed are then undefined.  (ptmi_ray_order_device's order is a permutation and qualifies; so does a list of live rays.)
 *   - Refusals enqueue and write nothing: PTMI_ESTATE before any scene is set (the two path entries); PTMI_EINVAL for a negative n or m,
 *     for a NULL required pointer with a positive count, and for a scene that holds a GLASS material -- render Inline cannot split rays,
 *     as for ptmi_render(PTMI_INLINE).
 *   - There is no group form, as for the ray queries. */
int ptmi_path_seeds_device(ptmi_ctx *ctx, uint64_t seed0, uint64_t first_index, int n, uint32_t *d_seed /* [n][4] */);
int ptmi_trace_paths_device(ptmi_ctx *ctx, const float *d_rays /* [n][6] */, int n, int bounce_limit, int n_spp,
                            float *d_color /* [n][3], in/out */, uint32_t *d_seed /* [n][4] a, b, c, counter; in/out */);
int ptmi_trace_paths_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m,
                                    int bounce_limit, int n_spp, float *d_color, uint32_t *d_seed);

/* ---- stepped paths: one bounce at a time, and the live rays -------------------- */
/* ptmi_trace_paths_device's loop is closed.  These entries hand a caller the one function that loop iterates and the list of rays that
 * are still alive, so that an integrator of the caller's own -- next-event estimation with ptmi_occluded_device between bounces, Russian
 * roulette, a depth limit per ray, per-bounce AOVs, a light tracer, a path that stops in a region -- keeps the device's materials,
 * rotation and SFC32 draws.  The order, lifetime and alignment rules are those of "ray queries on the device": everything is enqueued on
 * the context's launch stream, no host synchronisation, no device allocation, no copy to the host; a later scene call is ordered behind
 * the call; 4-byte alignment suffices for every array (8-byte aligned rays and hit records and 16-byte aligned seeds are moved in wider
 * pieces).  The context's state planes, partition, camera and statistics are not touched.  There is no group form.
 *   - ptmi_bounce_rays_device does, for ray i, exactly one prepareRay (src/Scene/Trace.hs:359-383) on (ray_i, radiance_i, throughput_i,
 *     seed_i), all four read and written in place, with the render kernels' own arithmetic:
 *       FROZEN OR MISSED -- nearZero throughput_i (the ray is then not traced; a NaN throughput is not nearZero), or checkHit scene ray_i
 *         is Nothing:  throughput_i = (0, 0, 0); ray, radiance and seed keep every bit; the optional outputs get the miss record
 *         (t 0, idx -1, six zeros).
 *       HIT -- computeRay:  radiance_i += emittance * throughput_i;  throughput_i *= tmod;  ray_i = (hit + next ^* epsilon, next);  the
 *         seed advances by genVec's draws; the optional outputs receive ptmi_trace_rays_device's words for the INCOMING ray: t, the
 *         primitive, and the position and normal that were shaded.
 *     So from throughput 1 and radiance 0, k calls give traceInline k's result (as 0 + radiance) and seed bit for bit, and
 *     ptmi_trace_paths_device(limit k, 1 spp) from a zero colour.  d_t, d_idx and d_hit may each be NULL.
 *   - ptmi_bounce_rays_indexed_device: lane k < m takes i = d_index[k]; an entry outside [0, n) is skipped, nothing is read or written for
 *     it; a position no entry names is left untouched.  The state is read, modified and written, so the index must name a ray AT MOST
 *     ONCE: a ray named twice is a race between two lanes.  (ptmi_ray_order_device's order and ptmi_live_rays_device's list qualify: the
 *     list's -1 padding is skipped.)
 *   - Refusals of the two step entries are those of ptmi_trace_paths_device, and nothing is enqueued or written: PTMI_ESTATE before any
 *     scene is set; PTMI_EINVAL for a negative n or m, for a NULL required pointer with a positive count, and for a scene that holds a
 *     GLASS material.  n == 0 or m == 0 is PTMI_OK and touches nothing.
 *   - ptmi_live_rays_device lists the rays that are still alive.  The candidates are d_index[0 .. m), or 0 .. n - 1 when d_index is NULL
 *     (m is then not looked at beyond its sign); a candidate is live when it lies in [0, n) and its throughput is not nearZero.  d_live
 *     receives the live candidates in candidate order -- the compaction is stable and deterministic, so a coherent order stays coherent
 *     -- and -1 in every remaining entry up to the candidate count; d_count, unless NULL, receives their number.  IN PLACE: d_live may be
 *     the same array as d_index (the candidates are copied into the workspace before the first entry is written); any other overlap is
 *     undefined.  d_work: ptmi_live_rays_bytes(candidate count) bytes, 8-byte aligned, scratch while the call is in flight.  It needs no
 *     scene (no PTMI_ESTATE).  Several small launches (count, scan, scatter), none of which waits on another workgroup.
 *     Refusals, nothing enqueued or written: PTMI_EINVAL for a negative n or m, for a NULL d_live or d_work or (with n > 0) d_throughput
 *     with a positive candidate count, for a d_work that is not 8-byte aligned, for work_bytes below ptmi_live_rays_bytes; PTMI_ELIMIT
 *     for a candidate count above PTMI_LIVE_RAYS_MAX.  Zero candidates is PTMI_OK and touches nothing.
 *   - ptmi_live_rays is its host twin: host arrays, no context, no device, no workspace; the same list, the same refusals, and `live`
 *     may be `index`.  It is the definition the device list is tested against. */
#define PTMI_LIVE_RAYS_MAX (1 << 22)
int ptmi_bounce_rays_device(ptmi_ctx *ctx, float *d_rays /* [n][6], in/out */, int n, float *d_throughput /* [n][3], in/out */,
                            float *d_radiance /* [n][3], in/out */, uint32_t *d_seed /* [n][4], in/out */,
                            float *d_t, int32_t *d_idx, float *d_hit /* [n][6]; each of the three may be NULL */);
int ptmi_bounce_rays_indexed_device(ptmi_ctx *ctx, float *d_rays, int n, const int32_t *d_index, int m, float *d_throughput,
                                    float *d_radiance, uint32_t *d_seed, float *d_t, int32_t *d_idx, float *d_hit);
size_t ptmi_live_rays_bytes(int count);   /* workspace for that many candidates; 0 for count <= 0 */
int ptmi_live_rays_device(ptmi_ctx *ctx, const float *d_throughput /* [n][3] */, int n, const int32_t *d_index /* [m] or NULL */, int m,
                          int32_t *d_live /* [m], or [n] when d_index is NULL */, int32_t *d_count /* one word, may be NULL */,
                          void *d_work, size_t work_bytes);
int ptmi_live_rays(const float *throughput, int n, const int32_t *index, int m, int32_t *live, int32_t *count);

/* ---- render Streams along a caller's rays -------------------------------------- */
/* The entries above are render Inline.  These run the library's other algorithm, render Streams (src/Scene/Trace.hs:141-191, 272-331), along
 * a caller's own device-resident rays: no bounce limit -- a path ends by nearZero, a miss or PTMI_OPT_STREAM_STEP_CAP -- the Streams seed
 * rule (PTMI_OPT_STREAMS_SEED_RULE), and rays that SPLIT: a scene with a GLASS material, which the Inline entries refuse, is served.
 * d_rays, d_color and d_seed are ptmi_trace_paths_device's arrays.  The order, lifetime and alignment rules are those of "ray queries on
 * the device": everything is enqueued on the context's launch stream, no host synchronisation, no device allocation, no copy; a later
 * scene call is ordered behind the call; 4-byte alignment suffices for rays, colour and seeds (8-byte aligned rays and 16-byte aligned
 * seeds are moved in wider pieces).  The context's state planes, partition, camera, dispatch order and ptmi_stats are not touched.
 *   - ptmi_trace_streams_device does for ray i what ptmi_render(PTMI_STREAMS) in its per-pixel form does for a pixel, with the render
 *     kernels' own arithmetic and the ray as given, with a direction of any length:
 *         acc = color_i ; pixel_seed = seed_i
 *         repeat n_spp times:
 *             cur = (ray_i, throughput (1, 1, 1), seed = pixel_seed, steps = 0) ; stack empty
 *             walk cur's ray tree depth first:
 *                 a lineage at steps >= step cap is cut and counted (truncated); otherwise checkHit, ++steps;
 *                 a hit:  acc = acc + emittance * throughput      (every hit, in walk order: one adder per colour word)
 *                         under PTMI_SEED_FROM_RESULT:  pixel_seed = the seed cur carried INTO this hit
 *                         nearZero throughput: the lineage ends
 *                         GLASS: the two children of the formula above (PTMI_GLASS); the refraction child waits on a stack of 16 (one
 *                                that finds it full is dropped and counted), the reflection child goes on; at steps >= step cap both
 *                                are cut
 *                         else:  calcNextRay; cut at steps >= step cap
 *                 a lineage that ends pops the most recent waiting child, else the sample is over
 *             pixel_seed advances one random @Float draw          (updateSeed)
 *         color_i = acc ; seed_i = pixel_seed
 *     The seed rule is the context's: PTMI_SEED_AUTO gives PTMI_SEED_FROM_RESULT without GLASS and PTMI_SEED_KEEP_ACCUMULATOR with it.  So
 *     the primary rays of a ptmi_camera, ptmi_path_seeds_device's seeds and the planes' colours give ptmi_init_output +
 *     ptmi_render(PTMI_STREAMS) with PTMI_FORM_PIXEL: all seven planes bit for bit, on every scene kind, with and without GLASS, under
 *     both seed rules; and one call of n_spp samples equals n_spp calls of one.
 *   - d_lost, unless NULL, is two 64-bit words, 8-byte aligned, ADDED to: [0] the rays the step cap cut (ptmi_stats'
 *     stream_rays_truncated), [1] the children a full stack dropped.  They receive one atomic add per wave, and only from a wave that
 *     lost something.
 *   - d_work holds the first waiting children of every lane, scratch while the call is in flight.  It is required, 16-byte aligned and
 *     at least ptmi_trace_streams_bytes(lanes) bytes only when the scene holds GLASS; without GLASS it is ignored and may be NULL.
 *     lanes is m with an index, else n.
 *   - ptmi_trace_streams_indexed_device follows ptmi_trace_paths_indexed_device's contract: lane k < m takes i = d_index[k]; an entry
 *     outside [0, n) is skipped, nothing is read or written for it; a position no entry names is left untouched.  Colour and seed are
 *     read, modified and written, so the index must name a ray AT MOST ONCE: a ray named twice is a race between two lanes.
 *   - Refusals enqueue and write nothing: PTMI_ESTATE before any scene is set; PTMI_EINVAL for a negative n or m, for a NULL required
 *     pointer with a positive count, for a d_lost that is not 8-byte aligned, for a d_work that is misaligned or shorter than
 *     ptmi_trace_streams_bytes(lanes) on a GLASS scene, and for GLASS with an explicit PTMI_SEED_FROM_RESULT, as for
 *     ptmi_render(PTMI_STREAMS).  n == 0, m == 0 or n_spp <= 0 is PTMI_OK and touches nothing.
 *   - There is no group form, as for the ray queries. */
size_t ptmi_trace_streams_bytes(int count);      /* workspace for that many lanes; 0 for count <= 0 */
int ptmi_trace_streams_device(ptmi_ctx *ctx, const float *d_rays /* [n][6] */, int n, int n_spp,
                              float *d_color /* [n][3], in/out */, uint32_t *d_seed /* [n][4], in/out */,
                              uint64_t *d_lost /* [2]: truncated, dropped; added to; may be NULL */,
                              void *d_work, size_t work_bytes);
int ptmi_trace_streams_indexed_device(ptmi_ctx *ctx, const float *d_rays, int n, const int32_t *d_index, int m, int n_spp,
                                      float *d_color, uint32_t *d_seed, uint64_t *d_lost, void *d_work, size_t work_bytes);

/* ---- point queries (the reference's unit-test surface) ------------------------ */
/* Evaluates distanceTo / hit (src/Scene/Intersection.hs:16-64) on the DEVICE for n independent
 * cases -- ray i against primitive i -- the way test/Scene/Intersection/Tests.hs:122-123
 * evaluates single expressions through the backend.  rays: n x 6 floats (origin, direction).
 * Outputs (host): is_just[n], t[n], hit_normalp[n x 6] (position, normal); the last may be NULL. */
int ptmi_eval_distance_to_sphere(ptmi_ctx *ctx, const ptmi_sphere *spheres, const float *rays, int n,
                                 int32_t *is_just, float *t, float *hit_normalp);
int ptmi_eval_distance_to_plane(ptmi_ctx *ctx, const ptmi_plane *planes, const float *rays, int n,
                                int32_t *is_just, float *t, float *hit_normalp);
/* checkHit (src/Scene/Trace.hs:443-447) on the DEVICE against the context's current scene, linear, BVH or mesh, for n host rays
 * (n x 6 floats: origin, direction): just_out[i] = 1 if ray i hits, then t_out[i] = its distance and idx_out[i] = the primitive
 * (spheres 0 .. n_spheres - 1, then planes, then triangles); for a miss t_out[i] = 0 and idx_out[i] = -1.  The same selection the render kernels make. */
int ptmi_eval_check_hit(ptmi_ctx *ctx, const float *rays, int n, float *t_out, int32_t *idx_out, int32_t *just_out);
/* sin/cos of the device math used by anglesToQuaternion, for pinning against libm. */
int ptmi_eval_sincos(ptmi_ctx *ctx, const float *x, int n, float *sin_out, float *cos_out);
/* anglesToQuaternion's second half (src/Util.hs:62-67) on the DEVICE, through the inline function the render kernels call: n host triples
 * of HALF angles (roll, pitch, yaw; n x 3 floats) -> q_out (n x 4 floats: w, x, y, z).  Inputs 64 k .. 64 k + 63 share a wave: the
 * kernels' three-angle sin/cos takes its fast form per wave, so a caller decides which angles vote together. */
int ptmi_eval_quaternion(ptmi_ctx *ctx, const float *half_angles, int n, float *q_out);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
