/* triangle_test.h -- TEST-ONLY: the device's triangle test (PTMI_TRIANGLE_TEST, csrc/ptmi_mesh_device.h) restated on the CPU, every operation
 * an f32 operation rounded on its own, on the record the host stores (mesh_traverse.c: mesh_records).  Shared by mesh_traverse.c (the
 * closest hit) and any_hit_traverse.c (occlusion); mesh_traverse.c's header comment spells the test out. */
#ifndef PTMI_TESTS_TRIANGLE_TEST_H
#define PTMI_TESTS_TRIANGLE_TEST_H

#include <math.h>

typedef struct { float x, y, z; } v3;

static inline v3 mk(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
static inline v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static inline v3 cross(v3 a, v3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

/* the record the host stores: vertices and the unit normal (NaN for zero area) */
typedef struct { v3 v0, v1, v2, n; } trec;

static inline int tri_test(const trec *r, v3 o, v3 d, float *t_out)
{
    const float denom = dot(d, r->n);
    const float t = dot(sub(r->v0, o), r->n) / denom;
    const v3 p = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);
    const float w0 = dot(cross(sub(r->v1, r->v0), sub(p, r->v0)), r->n);
    const float w1 = dot(cross(sub(r->v2, r->v1), sub(p, r->v1)), r->n);
    const float w2 = dot(cross(sub(r->v0, r->v2), sub(p, r->v2)), r->n);
    *t_out = t;
    return !(denom > 1e-6f) && !(t < 0.0f) && w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f && !isnan(r->n.x);
}

#endif
