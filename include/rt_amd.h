/*
 * rt_amd.h — C ABI of the MI355X-native render path.
 *
 * This is the drop-in boundary for the per-pixel render loop of
 * foriequal0/homework-18-graphics-raytracer.  The reference has no FFI: its
 * render loop is two rayon closures inside main() (src/main.rs:1090-1104 for
 * the Whitted pass, src/main.rs:1131-1156 for the distributed pass).  The seam
 * is created exactly there: everything those closures read (World, Camera,
 * width/height/depth literals) comes in as flat POD arrays, and everything they
 * produce (one LinSrgb per pixel) goes out as row-major f32 RGB.
 *
 * Plain pointers and sizes only; no C++/torch types.  Every function returns
 * RT_OK (0) or a negative rt_status and never unwinds or aborts the host
 * (the reference's convention is panic!/unwrap — src/main.rs:767-775,785 —
 * which cannot cross a C ABI).  rt_last_error() returns a thread-local message
 * for the last failing call.
 *
 * Threading (the reference shares `&World` immutably between rayon threads and
 * gives each pixel exclusive `&mut` access to its RNG, main.rs:1096, 1131):
 * an rt_scene is changed only by the rt_scene_update_* calls (below: the caller
 * orders them against renders on other streams) and may be rendered from several host threads at
 * once, each on its own HIP stream (per-(scene, stream) workspaces are created
 * under a lock; the rt_set_* settings are atomics; the profiling hooks keep the
 * event pair of a call in thread-local state).  Calls on ONE stream, and calls
 * on one rt_rng, must be serialised by the caller.
 *
 * State between calls: the per-(scene, stream) workspace remembers which frame
 * description it holds on the device, so that a call with the same frame as the
 * one before it is a single kernel launch.  A render call may be captured into a
 * HIP graph once its workspace exists (allocation cannot be captured: render the
 * frame once uncaptured first); from the first capture on a stream, every
 * launch on that stream prepares its own state, as the captured one does, since
 * replays come unannounced.
 */
#ifndef RT_AMD_H
#define RT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 1

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1, /* null pointer, empty frame, index out of range ... */
    RT_ERR_NO_DEVICE = -2,        /* no HIP device / HIP runtime failure at init */
    RT_ERR_HIP = -3,              /* a HIP call failed; rt_last_error() has hipGetErrorString */
    RT_ERR_OUT_OF_MEMORY = -4,
    RT_ERR_UNSUPPORTED = -5       /* e.g. max_depth above RT_MAX_DEPTH */
} rt_status;

/* Largest max_depth accepted by the render entry points (reference uses 5,
 * src/main.rs:1098,1139; the benchmark uses 8). */
#define RT_MAX_DEPTH 32

/* ---- scene model: flat mirrors of the reference's types ------------------- */

/* geometric.rs:42-47  PositionNormalUV { position, normal, uv } */
typedef struct rt_vertex {
    float position[3];
    float normal[3];
    float uv[2];
} rt_vertex;

/* primitives.rs:26-29  Triangle<PositionNormalUV> { object_index, vertices } */
typedef struct rt_triangle {
    uint32_t object_index; /* usize narrowed to u32 */
    rt_vertex vertices[3];
} rt_triangle;

/* primitives.rs:15-24  Sphere { object_index, geometry: { center, radius } } */
typedef struct rt_sphere {
    uint32_t object_index;
    float center[3];
    float radius;
} rt_sphere;

/* materials.rs:70-83 stores two Rust closures in GenerativeMaterial; closures
 * cannot cross a C ABI, so the closure bodies that exist in the reference
 * (src/main.rs:848-863 and 1019-1026) are enumerated. */
typedef enum rt_diffuse_fn {
    RT_DIFFUSE_CONST = 0,      /* ColorMaterial: diffuse_color                    (materials.rs:33-37) */
    RT_DIFFUSE_STRIPE_V = 1,   /* ((uv.y * f) as i32 % 2 == 0) ? tex_a : tex_b    (main.rs:848-854)   */
    RT_DIFFUSE_STRIPE_SUM = 2  /* (((uv.x + uv.y) * f) as i32 % 2 == 0) ? a : b   (main.rs:1019-1025) */
} rt_diffuse_fn;

typedef enum rt_normal_fn {
    RT_NORMAL_CONST = 0,       /* ColorMaterial.normal / |uv| (0,0,1)             (main.rs:1026)      */
    RT_NORMAL_WAVE_U = 1       /* a = uv.x*nf*2*PI; v=(sin a,0,cos a); v.z<=0 ? -v : v (main.rs:855-863) */
} rt_normal_fn;

/* materials.rs:21-31 ColorMaterial (14 f32) + the enumerated closure parameters */
typedef struct rt_material {
    uint32_t diffuse_fn;       /* rt_diffuse_fn */
    uint32_t normal_fn;        /* rt_normal_fn  */
    float normal[3];           /* tangent-space bump normal, (0,0,1) for flat */
    float diffuse_color[3];
    float shiness;
    float specular_color[3];
    float smoothness;
    float transparency;
    float refraction_index;
    float opaque_decay;
    float tex_color_a[3];      /* generative diffuse: colour when the cell index is even */
    float tex_color_b[3];      /*                     colour otherwise                   */
    float tex_frequency;       /* 20.0 (main.rs:849) / 10.0 (main.rs:1020) */
    float normal_frequency;    /* 10.0 (main.rs:856) */
} rt_material;

/* lights.rs:6-30 */
typedef enum rt_light_kind {
    RT_LIGHT_DIRECTIONAL = 0,
    RT_LIGHT_SPOT = 1,
    RT_LIGHT_POINT = 2
} rt_light_kind;

typedef struct rt_light {
    uint32_t kind;        /* rt_light_kind */
    uint32_t has_origin;  /* Directional.origin is Option<Point3> (lights.rs:8); Spot/Point always 1 */
    float origin[3];
    float direction[3];   /* Directional, Spot */
    float angle;          /* Spot: radians */
    float softness;       /* Spot */
    float color[3];
} rt_light;

/* src/main.rs:130-137 World { objects, triangles, spheres, lights }.
 * Array ORDER is semantically significant: nearest-hit ties resolve to the
 * later primitive (main.rs:229-233, 298-302) and lights are summed in order. */
typedef struct rt_scene_desc {
    const rt_triangle *triangles; uint32_t n_triangles;
    const rt_sphere   *spheres;   uint32_t n_spheres;
    const rt_material *materials; uint32_t n_materials; /* one per Object (primitives.rs:8-10) */
    const rt_light    *lights;    uint32_t n_lights;
} rt_scene_desc;

/* src/main.rs:43-49 */
typedef struct rt_camera {
    float fovy;       /* radians */
    float center[3];
    float toward[3];
    float up[3];
    float near;
} rt_camera;

/* Frame + tile.  The reference renders the full frame (main.rs:1084-1089);
 * the tile fields are what image-tile sharding over several GPUs needs.
 * Rendered pixels: x in [x0,x1), y in {y0, y0+y_step, ...} < y1.
 * Output is compact: out[((row * (x1-x0)) + (x - x0)) * 3 + c], row = (y-y0)/y_step.
 * With x0=y0=0, x1=width, y1=height, y_step=1 that is the reference's
 * row-major [y*width + x] (image.rs:35-47).  A tile must hold fewer than 2^32
 * pixels (RT_ERR_UNSUPPORTED otherwise: render it as several tiles). */
typedef struct rt_frame {
    uint32_t width, height;
    int32_t  max_depth;      /* TraceState.depth at the root (main.rs:1098); an i32 tested with `depth <= 0`
                              * (main.rs:488, 669), so a negative value renders like 0, as in the reference */
    uint32_t x0, y0, x1, y1;
    uint32_t y_step;         /* >= 1 */
} rt_frame;

typedef struct rt_scene rt_scene; /* opaque: device-resident; changed only by the rt_scene_update_* calls */

/* ---- entry points --------------------------------------------------------- */

/* ABI version of the loaded library (== RT_ABI_VERSION it was built with). */
int rt_abi_version(void);

/* Thread-local message for the last failing call on this thread ("" if none). */
const char *rt_last_error(void);

/* Number of HIP devices visible, or a negative rt_status. */
int rt_device_count(void);

/* Select the HIP device used by subsequent calls on this thread. */
int rt_set_device(int device);

/* Number of rows / pixels a frame's tile covers (host arithmetic only). */
uint32_t rt_frame_rows(const rt_frame *frame);
uint64_t rt_frame_pixels(const rt_frame *frame);

/* Upload a scene to the current device.  Replaces the construction of `World`
 * (src/main.rs:811-1075) as seen by the render loop: the library precomputes
 * the per-triangle face normal and plane constant (primitives.rs:36-47,
 * main.rs:202-203; pure functions of the vertices, so bit-identical to the
 * reference's per-ray recomputation) and owns the device copy until destroy. */
int rt_scene_create(const rt_scene_desc *desc, rt_scene **out_scene);
int rt_scene_destroy(rt_scene *scene);

/* Whitted pass over one tile: replaces the par_iter closure at
 * src/main.rs:1090-1104 (shoot -> ray_trace(depth, contribution 1.0)).
 *   d_rgb        device pointer, rt_frame_pixels(frame)*3 floats, linear radiance
 *                BEFORE post_process (what ray_trace returns, main.rs:1101-1102).
 *   d_ray_count  device pointer to one u64 or NULL; the number of World::cast
 *                evaluations performed is ADDED to it (the reference only counts
 *                pixels, main.rs:1108).
 *   hip_stream   hipStream_t (as void*), NULL = default stream.  The launch is
 *                stream-ordered and asynchronous. */
int rt_render_whitted(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame,
                      float *d_rgb, unsigned long long *d_ray_count, void *hip_stream);

/* Same, with host buffers: allocates, launches, copies back and synchronises.
 * *h_ray_count is overwritten with the cast count of this call (may be NULL). */
int rt_render_whitted_host(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame,
                           float *h_rgb, unsigned long long *h_ray_count);

/* ---- ray queries: World::cast on caller-supplied rays ------------------------------

 * World::cast (src/main.rs:180-326) for a batch of unrelated rays: "what does this ray hit?" — picking, visibility between two
 * points, a depth / normal / object-id buffer, rays of a camera model the library does not have.  Every result is bit-identical
 * to the reference's cast of that ray, NaN distances included. */

/* main.rs:69-81 Ray + Option<Exclusion>, flattened */
typedef struct rt_ray {
    float origin[3];
    float direction[3];      /* used as given: not normalised (the reference does not normalise in cast) */
    uint32_t face_direction; /* 0 Front, 1 Back, 2 Both (main.rs:52-57); a value above 2 is read as Both */
    uint32_t has_exclude;    /* 0: None; anything else: Some */
    uint32_t exclude_kind;   /* 0 Sphere, 1 Triangle (PrimitiveIndex, primitives.rs:31-34); any other kind excludes nothing */
    uint32_t exclude_index;  /* index into the scene's sphere or triangle array; beyond that array it excludes nothing, as in the
                              * reference, where PrimitiveIndex equality simply never holds */
    uint32_t exclude_face;   /* 0 Front, 1 Back, 2 Both; a value above 2 is read as Both */
} rt_ray;                    /* 44 bytes */

/* main.rs:139-147 Hit, flattened */
#define RT_HIT_NONE 0xffffffffu
typedef struct rt_hit {
    uint32_t kind;           /* 0 Sphere, 1 Triangle, RT_HIT_NONE: cast returned None (every other field 0) */
    uint32_t index, object_index; /* the primitive's index in its array (sphere or triangle), its Object's index */
    float position[3], normal[3], uv[2]; /* a sphere hit always carries its uv (main.rs:310-313) */
    uint32_t face_direction; /* 0 Front, 1 Back */
    float distance;
} rt_hit;                    /* 52 bytes */

/* For every ray d_rays[i], d_hits[i] = World::cast(ray) (device pointers, n_rays records each).  Stream-ordered and asynchronous
 * on hip_stream (NULL = default stream).  n_rays == 0 launches nothing; n_rays >= 2^32 is RT_ERR_UNSUPPORTED (checked first).
 * Graph capture: on a scene below the breadth-first switch (RT_AMD_BFS_WALK_TRIANGLES) the call uses no workspace and may be
 * captured at once.  A scene walked breadth-first keeps record lists in the per-(scene, stream) workspace, shared with
 * rt_render_whitted: make one uncaptured call on the stream first (with at least as many rays); a call captured before that
 * uses the pair-wise kernel, which gives the same results more slowly. */
int rt_cast_rays(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, rt_hit *d_hits, void *hip_stream);
/* Same, with host buffers: allocates, launches, copies back and synchronises. */
int rt_cast_rays_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, rt_hit *h_hits);
/* The primary rays Camera::shoot(clip(x, y)) (main.rs:83-99, 1093-1096) of every pixel of a frame or tile, in the tile's compact
 * row order (as the render output): d_rays[row * (x1 - x0) + (x - x0)], rt_frame_pixels(frame) records.  Face Front, no
 * exclusion; each ray is bit for bit the primary ray the Whitted pass casts.  frame->max_depth is not used.  Stream-ordered. */
int rt_camera_rays(const rt_camera *camera, const rt_frame *frame, rt_ray *d_rays, void *hip_stream);

/* ---- radiance queries: ray_trace on caller-supplied rays ------------------------------

 * ray_trace (src/main.rs:466-519) for every ray: d_rgb[3*i + c] = ray_trace(world, d_rays[i], TraceState { depth: max_depth,
 * contribution }) — the Whitted render with the caller's rays as its roots: a camera model the library does not have (a 360-degree,
 * fisheye, orthographic or stereo view), a re-render of chosen pixels, the secondary rays of the caller's own integrator.
 * Device pointers (n_rays records, 3 * n_rays floats); stream-ordered and asynchronous on hip_stream (NULL = default stream).
 *   value        ray_trace's own return value, bit for bit, NaN included.  It is NOT `0.0 + value` as a frame stores it
 *                (main.rs:1107; rt_render_whitted), so a -0.0 channel stays -0.0: rt_trace_rays(rt_camera_rays(frame)) + 0.0f
 *                equals rt_render_whitted(frame) bit for bit.
 *   d_rays       rt_ray records read exactly as rt_cast_rays reads them: a face value above 2 is Both, an exclusion whose index is
 *                outside its array excludes nothing, the direction is used as given.
 *   max_depth    as rt_frame.max_depth: negative renders like 0, above RT_MAX_DEPTH is RT_ERR_UNSUPPORTED.
 *   contribution the roots' TraceState.contribution, ray_trace's entry check included (below THRESHOLD = 0.001: black, no cast,
 *                main.rs:469).  Any float, NaN included (it passes the check and no child or shade is wanted: black, one cast).
 *   d_ray_count  NULL or one u64 device word: the call's World::cast count is ADDED to it (the sum over the rays of what the
 *                recursion of each casts).
 * Checked before any device work, in this order: n_rays >= 2^32 is RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT;
 * n_rays == 0 is RT_OK and launches nothing; a null ray or rgb pointer RT_ERR_INVALID_ARGUMENT; then max_depth.
 * Workspace and graph capture as rt_render_whitted: the call shares the per-(scene, stream) workspace, and may be captured after
 * one uncaptured call on that stream.  rt_profile_enable / rt_profile_read bracket its render kernel(s) as rt_render_whitted's.
 * Speed depends on the ORDER of the rays: the kernels cast 64 consecutive rays per wave, wave-uniformly, so rays that travel
 * together should be neighbours (rt_camera_rays' row order makes 64x1 strips; an 8x8-tile order is what rt_render_whitted uses;
 * DESIGN.md §3.8).  The stochastic integrator on caller rays is rt_trace_rays_distributed, below.  Not covered: per-ray cast counts. */
int rt_trace_rays(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, int32_t max_depth, float contribution,
                  float *d_rgb, unsigned long long *d_ray_count, void *hip_stream);
/* Same, with host buffers: allocates, launches, copies back and synchronises.  *h_ray_count is overwritten with the cast count
 * of this call (may be NULL).  Without a device it fails with a status and writes nothing into h_rgb. */
int rt_trace_rays_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, int32_t max_depth, float contribution,
                       float *h_rgb, unsigned long long *h_ray_count);

/* ---- hit queries: get_shade, get_reflect and get_refract on caller-supplied hits ------------------------------

 * What the reference does with a Hit once it holds one — the three calls ray_trace makes between two casts (main.rs:478-514) — so that
 * a caller can write the recursion itself, level by level: cast -> shade / reflect / refract -> cast, weighting, stopping, re-sorting
 * or mixing levels as it likes (INTEGRATION.md shows the loop).  A hit is the rt_hit rt_cast_rays writes; Hit.ray (main.rs:142)
 * travels beside it as the rt_ray that produced it: entry i of d_incoming belongs to entry i of d_hits.  Device pointers, n records
 * each; stream-ordered and asynchronous on hip_stream (NULL = default stream); no workspace, so every call may be captured into a
 * HIP graph at once, as rt_cast_rays below the breadth-first switch.  Every result is the reference's, bit for bit.
 * Records are the caller's and are validated, never trusted:
 *   - a hit whose kind is neither 0 nor 1, or (rt_shade_hits, rt_refract_rays) whose object_index >= n_materials, is "no hit": black,
 *     an all-zero ray, kind RT_HIT_NONE, and no cast; rt_reflect_rays has no scene and tests the kind only;
 *   - a hit's index outside its primitive array is used as given: it only serves as an exclusion, and as one excludes nothing (the
 *     rule of rt_ray.exclude_index);
 *   - a hit's face_direction above 1 is read as Back;
 *   - incoming rays are read exactly as rt_cast_rays reads them (a face value above 2 is Both); NaN and Inf in positions, normals or
 *     directions pass through the arithmetic as in the reference.
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT (rt_shade_hits,
 * rt_refract_rays); n == 0 is RT_OK and launches nothing; a null hits, incoming or required output pointer RT_ERR_INVALID_ARGUMENT.
 * A wave takes 64 consecutive records; a batch of more than 2^26 runs in bands of whole 64-record chunks (any n below 2^32).  The casts are pair-wise
 * (cast_pairs), or wave-uniform under RT_AMD_QUERY_WAVE_UNIFORM=1, with the same bits (DESIGN.md §3.10 says which is faster when).
 * A scene walked breadth-first (RT_AMD_BFS_WALK_TRIANGLES) gives the same bits through the same two casts: the breadth-first walk
 * itself is not used inside these kernels.
 * Not covered: per-record cast counts; rt_multi_* variants; the breadth-first walk inside these kernels (for get_shade's shadow casts it
 * comes with the light queries below, for get_refract's casts with the refraction queries after them: both hand their rays to
 * rt_cast_rays_indexed); the ray of Refraction::Infinite (main.rs:154-156), which the reference's callers discard (the refraction
 * queries keep it, and count casts per record). */

/* get_shade(&hit) (main.rs:407-464): d_rgb[3*i + c], bit for bit, NaN and -0.0 included.  d_ray_count: NULL or one u64 device word, the
 * shadow casts (one per light that faces the bumped normal, main.rs:435) are ADDED. */
int rt_shade_hits(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float *d_rgb,
                  unsigned long long *d_ray_count, void *hip_stream);
/* get_reflect(&hit) (main.rs:328-341): origin = the hit's position, direction normalised as the reference does, face mode = the incoming
 * ray's, exclusion { hit.kind, hit.index, invert(hit.face_direction) }.  Pure: needs no scene. */
int rt_reflect_rays(const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_ray *d_out, void *hip_stream);
/* get_refract(&hit, max_distance) (main.rs:343-405; the reference passes 100.0): 1 to 11 casts per hit.
 *   d_kind[i]    0 Escaped, 1 Infinite, 2 Trapped (main.rs:149-158), RT_HIT_NONE for a record that is no hit
 *   d_travel[i]  travel_distance when Escaped, else 0 (may be NULL)
 *   d_escape[i]  escape_ray when Escaped, else all-zero words; feeds rt_cast_rays / rt_trace_rays as it is
 *   d_ray_count  NULL or one u64 device word: the casts get_refract made are ADDED. */
int rt_refract_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float max_distance,
                    uint32_t *d_kind, float *d_travel, rt_ray *d_escape, unsigned long long *d_ray_count, void *hip_stream);
/* The same two with host buffers: allocate, launch, copy back and synchronise.  *h_ray_count is overwritten with the cast count of
 * this call (may be NULL).  Without a device they fail with a status and write nothing. */
int rt_shade_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float *h_rgb,
                       unsigned long long *h_ray_count);
int rt_refract_rays_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, float max_distance,
                         uint32_t *h_kind, float *h_travel, rt_ray *h_escape, unsigned long long *h_ray_count);

/* ---- light queries: get_shade light by light on caller-supplied hits ------------------------------

 * get_shade (main.rs:407-464) opened into the calls between its casts.  rt_shade_hits runs the whole light loop in one kernel, shadow
 * casts inside, and returns the sum; here the shadow rays are records like every other ray, so that a caller can touch direct
 * lighting — per-light output, a subset of lights (light linking), a shadow rule of its own (a jittered shadow ray, a shadow that
 * ignores glass), a re-weighting of diffuse against specular — and so that the shadow casts go through rt_select_records +
 * rt_cast_rays_indexed, which on a scene walked breadth-first take that walk.  The sequence, per range of lights,
 *     rt_light_rays -> rt_select_records(d_asks) -> rt_cast_rays_indexed(d_shadow_rays -> d_shadow_hits) -> rt_light_terms -> rt_light_fold
 * on a zeroed d_rgb gives rt_shade_hits' values and cast count bit for bit (INTEGRATION.md writes it out; DESIGN.md §3.14 says why the
 * bits are the same).  Records are the hit queries': entry i of d_incoming is Hit.ray of d_hits[i]; every pointer is a device pointer;
 * every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is one kernel with one record per lane, uses no
 * workspace and may be captured into a HIP graph at once.
 * Per-(light, record) arrays are light-major: entry k = (l - light_first) * n + i, n * light_count entries — one light's plane is
 * contiguous, and the whole array is one batch of n * light_count records for rt_select_records and rt_cast_rays_indexed.
 * The record rules are those of the hit-query block: a hit whose kind is neither 0 nor 1, or whose object_index >= n_materials, is "no
 * hit" — asks 0, an all-zero ray, lit 0, black, nothing cast, and its d_rgb entry is not written; a primitive index outside its array
 * only ever serves as an exclusion; a face above 1 reads as Back; NaN and Inf pass through the arithmetic.
 * Checked before any device work, in this order: n >= 2^32, or n * light_count >= 2^32, is RT_ERR_UNSUPPORTED; a null scene
 * RT_ERR_INVALID_ARGUMENT; n == 0 or light_count == 0 is RT_OK and launches nothing; a null required pointer RT_ERR_INVALID_ARGUMENT; only
 * then is the scene read: light_first + light_count > n_lights (in 64 bits) is RT_ERR_INVALID_ARGUMENT.
 * Not covered: _host forms (the calls sit between device calls); rt_multi_* forms; per-record cast counts. */

/* main.rs:408-433 per record and light, with material = approx(hit.at) and normal = adjust_normal(hit.at.normal):
 *   d_asks[k]            1 where approximate_into_directional is Some and !(cosine <= 0) — a NaN cosine asks, as in the reference —
 *                        else 0: exactly the pairs rt_shade_hits casts a shadow ray for
 *   d_shadow_rays[k]     where the light asks, shadow_ray: origin = the hit's position, direction = -light.direction, face Back,
 *                        exclusion { hit.kind, hit.index, Back } — bit for bit the ray rt_shade_hits casts; elsewhere all-zero words
 *   d_light_distance[k]  (may be NULL) what main.rs:439 compares against: the distance from the hit to the light's origin, +inf for a
 *                        directional light without origin, 0 where the light does not ask.  For a caller's own occlusion rule;
 *                        rt_light_terms does not read it. */
int rt_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                  rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_light_distance, void *hip_stream);
/* main.rs:435-459.  d_shadow_hits[k] — what a cast of d_shadow_rays[k] wrote — is read only where d_asks[k] != 0, so it needs no preset.
 * The occlusion rule is the reference's: a shadow hit of kind 0 or 1 occludes a light without origin always, and a light with origin
 * where distance(hit.position, shadow_hit.position) < distance(hit.position, light.origin); any other kind is a miss.
 *   d_lit[k]             1 where the record is a hit, d_asks[k] != 0, approximate_into_directional is Some and the light is not occluded
 *   d_diffuse[3k ..], d_specular[3k ..]   there, the locals `diffuse` and `specular` of main.rs:458-459: get_diffuse / get_specular of the
 *                        probe times light.color, not yet weighted by shiness; elsewhere d_lit[k] = 0 and both are +0
 * The probe's light_direction is -light.direction of the light itself, not the direction of d_shadow_rays[k]: a caller may have
 * replaced that ray.  d_asks is the caller's and is not trusted: a flag set where the light would not have asked costs nothing unsafe
 * (None gives d_lit[k] = 0; a cosine that is not positive makes get_diffuse and get_specular black by their own tests). */
int rt_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                   const unsigned char *d_asks, const rt_hit *d_shadow_hits, unsigned char *d_lit, float *d_diffuse, float *d_specular,
                   void *hip_stream);
/* main.rs:461: for l = 0 .. light_count - 1 in order, where d_lit[l * n + i]:
 *     rgb = (rgb + diffuse * (1 - shiness)) + specular * shiness        per channel, in place on d_rgb[3i ..]
 * with the shiness of the hit's material; every operation rounds to f32 and none is fused.  The call ADDS: the caller zeroes d_rgb
 * before the first range of lights, as `sum` starts black, and later ranges continue the same sum — a fold over ranges of lights in
 * order is the fold over all of them.  "No hit" records are not written.  It takes no light_first: it reads the material only. */
int rt_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, const unsigned char *d_lit, const float *d_diffuse,
                  const float *d_specular, float *d_rgb, void *hip_stream);

/* ---- area-light queries: soft shadows from sampled lights on caller-supplied hits ------------------------------

 * The light queries above on lights that have a size.  Every light of the reference is a point, so every shadow has a hard edge; here
 * a light l with radius rad is a sphere around its origin (around the tip of its direction, for a directional light without origin),
 * each (record, light) pair is evaluated spp times, each time with the light displaced to a point chosen on that sphere, and the fold
 * averages a light's samples before it weights and sums the lights — the noisy input the film, temporal, variance-guided and
 * upsampling queries below are there to clean.  The sequence, per range of lights,
 *     rt_area_light_rays -> rt_select_records(d_asks) -> rt_cast_rays_indexed(d_shadow_rays -> d_shadow_hits) -> rt_area_light_terms
 *         -> rt_area_light_fold
 * with every radius 0 and spp 1 is the light queries' sequence bit for bit, and therefore rt_shade_hits (INTEGRATION.md writes it out;
 * DESIGN.md §3.29 says why).  With a radius above 0 every value is what rt_light_rays / rt_light_terms give for the scene whose light
 * has been moved to the sample; the same arguments give the same bits on every run.
 *
 * The sample.  (record id, absolute light index l, sample number s in 0 .. spp - 1) name a point on the unit sphere, in single f32
 * operations in this order, none fused (csrc/rt_area_light.h, shared by both libraries; film_mix and film_offset are the film
 * queries', rtdm::sinf / cosf / f_sqrt csrc/rt_detmath.h's):
 *     seed_l = film_mix(seed ^ (0x9e3779b9u * (l + 1u)))
 *     u_a    = film_offset(pattern, k, id, seed_l, s, a) + 0.5f        a = 0, 1;  k = the side of a stratified pattern, spp = k * k
 *     z      = 1.0f - 2.0f * u_0
 *     r      = sqrt(max(1.0f - z * z, 0.0f))                           correctly rounded
 *     phi    = 6.2831855f * u_1
 *     offset = (r * cosf(phi), r * sinf(phi), z)
 * which is uniform on the sphere.  pattern is RT_FILM_UNIFORM or RT_FILM_STRATIFIED (spp = k * k, 1 <= k <= 8: one sample per cell of
 * the k x k grid over (u_0, u_1)); RT_FILM_CENTER is refused; 1 <= spp <= 64.  The displaced light of radius rad:
 *   - !(rad > 0) — zero, negative, NaN: the light exactly as stored; nothing is added to any of its words, and the sample is the
 *     stored origin (the stored direction, for a directional light without origin);
 *   - a light with an origin (spot, point, directional with has_origin): origin' = origin + offset * rad, per component the product,
 *     then the add; every other field unchanged;
 *   - a directional light without origin: direction' = normalize(direction + offset * rad).
 *
 * Per-entry arrays are sample-major, then light-major: entry k = (s * light_count + (l - light_first)) * n + i,
 * spp * light_count * n entries — one (sample, light) plane is contiguous, and the whole array is one batch of records for
 * rt_select_records and rt_cast_rays_indexed.  The record rules are those of the light queries.  Every pointer is a device pointer;
 * every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is one kernel with one record per lane,
 * allocates nothing, uses no workspace and may be captured into a HIP graph at once.
 * Checked before any device work, in this order: n >= 2^32, n * light_count >= 2^32 or n * light_count * spp >= 2^32 is
 * RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT; n == 0 or light_count == 0 is RT_OK and launches nothing; a null required
 * pointer RT_ERR_INVALID_ARGUMENT; spp outside 1 .. 64, RT_FILM_CENTER, an unknown pattern or a stratified spp that is no square
 * RT_ERR_INVALID_ARGUMENT with a message that names the limit; only then is the scene read: light_first + light_count > n_lights.
 * Not covered: _host forms of these three (they sit between device calls; the sampler alone has a CPU form, rt_area_light_samples_cpu
 * of include/rt_host.h); rt_multi_* forms; area lights inside rt_render_whitted; importance sampling towards the hit or an emitter
 * that is no sphere — for those a caller writes d_sample itself. */

/* rt_light_rays on the displaced lights.  d_radii: light_count floats, the radius of light light_first + j at j.  d_ids: n u32, the
 * record id of the hash — the global pixel index, say, so that a pixel draws the same points wherever it lies in the batch — or NULL
 * for id = (uint32_t)i.
 *   d_sample[3k ..]      the displaced origin, or the displaced direction for a directional light without origin; written for every
 *                        entry, whether the light asks or not, "no hit" records included
 *   d_asks[k], d_shadow_rays[k]   what rt_light_rays gives for the displaced light: the ray starts at the hit and runs along
 *                        -direction of the displaced light, face Back, exclusion { hit.kind, hit.index, Back }; all-zero words where
 *                        the light does not ask */
int rt_area_light_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                       const float *d_radii, const uint32_t *d_ids, uint32_t spp, uint32_t pattern, uint32_t seed, rt_ray *d_shadow_rays,
                       unsigned char *d_asks, float *d_sample, void *hip_stream);
/* rt_light_terms with the light replaced by a copy whose origin — direction, for a directional light without origin — is d_sample[3k ..]:
 * the occlusion distance is measured to that origin, and approximate_into_directional, get_diffuse and get_specular see that light.
 * It takes no radii and no seed: d_sample is the caller's, and may hold points of its own (a quad light, another sampling scheme). */
int rt_area_light_terms(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, uint32_t light_first, uint32_t light_count,
                        uint32_t spp, const unsigned char *d_asks, const float *d_sample, const rt_hit *d_shadow_hits, unsigned char *d_lit,
                        float *d_diffuse, float *d_specular, void *hip_stream);
/* Per record, for l = 0 .. light_count - 1 in order: over the samples s = 0 .. spp - 1 in order where d_lit[k], acc starts as the first
 * lit sample's term and every later lit term is added to it, for diffuse and specular separately; a light without a lit sample is
 * skipped, as rt_light_fold skips an unlit light; otherwise D = acc_d / (float)spp, S = acc_s / (float)spp and
 *     rgb = (rgb + D * (1 - shiness)) + S * shiness                     per channel, in place on d_rgb[3i ..]
 * Every operation rounds to f32 and none is fused.  The call ADDS, as rt_light_fold does; "no hit" records are not written.
 *   d_visibility         NULL, or light_count * n floats: entry l * n + i is (float)(lit samples) / (float)spp, 0 for a "no hit"
 *                        record — the shadow mask of light l, for a denoiser */
int rt_area_light_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t light_count, uint32_t spp, const unsigned char *d_lit,
                       const float *d_diffuse, const float *d_specular, float *d_rgb, float *d_visibility, void *hip_stream);

/* ---- hemisphere queries: ambient occlusion and one bounce of diffuse light on caller-supplied hits ------------------------------

 * get_shade lights a hit from the stored lights alone: no ambient term, no light from other surfaces, black where no light asks
 * (the `continue`s at main.rs:407).  This block samples the hemisphere over a hit with cosine-distributed directions and folds what
 * comes back along them into two products: ambient occlusion — a plane that a compositor or a denoiser multiplies an ambient or sky
 * colour by — and one bounce of diffuse inter-reflection, the radiance rt_trace_rays returns along the directions weighed by the
 * hit's diffuse colour.  Both are noisy; the film, temporal, variance-guided and upsampling queries below are there to clean them.
 *     ambient occlusion   rt_hemisphere_rays -> rt_select_records(d_asks) -> rt_cast_rays_indexed(d_rays -> d_shadow_hits)
 *                             -> rt_hemisphere_fold(d_shadow_hits, max_distance -> d_ambient)
 *     one bounce          rt_hemisphere_rays -> rt_trace_rays(d_rays -> d_radiance, all spp * n of them) -> rt_hemisphere_fold(d_radiance -> d_rgb)
 * (INTEGRATION.md writes both out)
 *
 * The sample.  (record id, sample number s in 0 .. spp - 1) name a direction, in single f32 or u32 operations in this order, none
 * fused (csrc/rt_hemisphere.h, shared by both libraries; film_mix and film_offset are the film queries', rtdm::sinf / cosf / f_sqrt
 * csrc/rt_detmath.h's, adjust_normal csrc/rt_shade.h's — the reference's Quaternion::from_arc(+z, N) applied to a vector):
 *     seed_h = film_mix(seed ^ 0x85ebca6bu)                            a stream of its own, apart from the area lights'
 *     u_a    = film_offset(pattern, k, id, seed_h, s, a) + 0.5f        a = 0, 1;  k = the side of a stratified pattern, spp = k * k
 *     r      = sqrt(u_0)                                               correctly rounded
 *     z      = sqrt(max(1.0f - u_0, 0.0f))
 *     phi    = 6.2831855f * u_1
 *     local  = (r * cosf(phi), r * sinf(phi), z)                       cosine-distributed about +z (Malley)
 *     dir    = adjust_normal(local, N)
 * N is chosen by normal_kind: RT_HEMISPHERE_SHADING is adjust_normal(material.normal, hit.normal) — the normal get_shade lights with,
 * rt_material_hits' shading_normal bit for bit; RT_HEMISPHERE_GEOMETRIC is hit.normal.  pattern is RT_FILM_UNIFORM or
 * RT_FILM_STRATIFIED (spp = k * k, 1 <= k <= 8: one sample per cell of the k x k grid over (u_0, u_1)); RT_FILM_CENTER is refused;
 * 1 <= spp <= 64.  A stratified u_0 may round to exactly 1: then z is 0, the direction lies in the tangent plane and does not ask.
 *
 * Per-entry arrays are sample-major: entry k = s * n + i, spp * n entries — one sample's plane is contiguous, and the whole array is
 * one batch of records for rt_select_records, rt_cast_rays_indexed and rt_trace_rays.  The record rules are those of the hit queries.
 * Every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is one
 * kernel with one record per lane, allocates nothing, uses no workspace and may be captured into a HIP graph at once.
 * Checked before any device work, in this order: n >= 2^32 or n * spp >= 2^32 is RT_ERR_UNSUPPORTED; a null scene
 * RT_ERR_INVALID_ARGUMENT; n == 0 is RT_OK and launches nothing; a null required pointer RT_ERR_INVALID_ARGUMENT; spp outside
 * 1 .. 64, RT_FILM_CENTER, an unknown pattern, a stratified spp that is no square or an unknown normal_kind RT_ERR_INVALID_ARGUMENT
 * with a message that names the limit; only then is the scene read.
 * Not covered: _host forms of these two (they sit between device calls; rt_hemisphere_dirs_cpu and rt_hemisphere_fold_cpu of
 * include/rt_host.h are the CPU forms); rt_multi_* forms; hemisphere sampling inside rt_render_*; other distributions — the
 * surface's Phong lobes are the lobe queries' below, for any other a caller overwrites d_dirs and d_rays; more than one bounce. */
#define RT_HEMISPHERE_SHADING 0u   /* N = adjust_normal(material.normal, hit.normal) */
#define RT_HEMISPHERE_GEOMETRIC 1u /* N = hit.normal */

/* d_ids: n u32, the record id of the hash — the global pixel index, say, so that a pixel draws the same directions wherever it lies
 * in the batch — or NULL for id = (uint32_t)i.
 *   d_dirs[3k ..]   dir, for every entry of a record that is a hit; zero words for a "no hit" record
 *   d_asks[k]       !(dot(dir, N) <= 0) on a hit, else 0
 *   d_rays[k]       the shadow ray get_shade builds (main.rs:425-433) with -light.direction = dir: origin hit.position, direction dir,
 *                   face Back, exclusion { hit.kind, hit.index, Back }; all-zero words where d_asks[k] is 0, as with rt_light_rays
 * — which is rt_light_rays for a directional light without origin whose direction is -dir, bit for bit.  A Back ray is answered by
 * back faces only (main.rs:185): occluders are closed objects, as for every shadow ray of the reference. */
int rt_hemisphere_rays(const rt_scene *scene, const rt_hit *d_hits, size_t n, const uint32_t *d_ids, uint32_t spp, uint32_t pattern, uint32_t seed,
                       uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs, void *hip_stream);
/* Per record, over the samples s = 0 .. spp - 1 in order:
 *     open[k] = d_asks[k] && !(d_shadow_hits[k] is a hit && distance(hit.position, d_shadow_hits[k].position) < max_distance)
 * with rt_light_terms' f32 distance.  max_distance = +inf makes every answered cast at a finite distance occlude (the directional
 * rule); a NaN distance leaves the sample open (the point-light compare); d_shadow_hits NULL: open = d_asks.  d_shadow_hits[k] is
 * read only where d_asks[k] is set.  On a "no hit" record every flag is 0.
 *   d_open       NULL, or spp * n bytes: open[k]
 *   d_ambient    NULL, or n floats: (float)(open samples) / (float)spp, 0 for a "no hit" record
 *   d_rgb, d_radiance   both NULL, or n * 3 floats and spp * n * 3 floats (what rt_trace_rays wrote for d_rays, say): over s where
 *                d_asks[k] is set, acc starts as the first such radiance and every later one is added to it; a record with none adds
 *                nothing; otherwise E = acc / (float)spp and
 *                    rgb = rgb + (diffuse_color * E) * (1 - shiness)          per channel, in place on d_rgb[3i ..]
 *                with the material's values as get_shade reads them.  Every operation rounds to f32 and none is fused.  The call
 *                ADDS, as rt_light_fold does; "no hit" records are not written.  The radiance of an entry that did not ask is never
 *                read. */
int rt_hemisphere_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t spp, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                       float max_distance, const float *d_radiance, unsigned char *d_open, float *d_ambient, float *d_rgb, void *hip_stream);

/* ---- environment queries: a lat-long sky for the rays that found nothing, and sky light on caller-supplied hits ----------------

 * A ray that leaves the scene is black (main.rs:475), and a hit is lit by the stored lights alone.  This block adds the sky: an
 * environment map that answers the rays which found nothing, and that lights a hit through directions drawn in proportion to its
 * brightness.  The environment is a caller-owned device image of height x width x 3 f32, linear RGB, row-major, row 0 at the zenith,
 * equirectangular with y up (the reference scene's camera).  Texel-space point (x_f, y_f) lies in the direction
 *     theta = 3.1415927f * y_f / (float)H     phi = 6.2831855f * x_f / (float)W + rotation
 *     dir   = (sin theta * cos phi, cos theta, sin theta * sin phi)
 * with rtdm::sincosf, every operation a single f32 one in the order written, none fused (csrc/rt_environment.h, shared by both
 * libraries).  The sequences
 *     the sky behind a batch   rt_cast_rays -> rt_environment_lookup(d_hits)
 *     the sky in the tree loop rt_tree_fold of a level -> rt_environment_lookup(the level's rays, hits, count and parent links), before
 *                              the parent level folds: it replaces the +0 the fold wrote for the level's misses
 *     sky light on hits        rt_environment_table (once per image) -> rt_environment_rays -> rt_select_records(d_asks) ->
 *                              rt_cast_rays_indexed(d_rays -> d_shadow_hits) -> rt_material_hits + rt_probe_surfaces(d_dirs, n_probes = spp)
 *                              -> rt_environment_fold
 * are written out in INTEGRATION.md; DESIGN.md §3.32 has what they cost.
 *
 * The lookup.  d = dir / |dir| (|dir| = sqrt of the f32 dot product; a length that is 0, NaN or Inf — a zero or non-finite
 * direction — gives +0), theta = acosf(min(max(d.y, -1), 1)), phi = atan2f(d.z, d.x) - rotation, x_f = phi * W / 6.2831855f,
 * x_f = x_f - floorf(x_f / W) * W, y_f = theta * H / 3.1415927f, both clamped to [0, W] and [0, H].  RT_ENV_NEAREST: x = min((uint32)x_f,
 * W - 1), y likewise, rgb = texel(x, y) * scale.  RT_ENV_BILINEAR: texel centres at + 0.5 — xs = x_f - 0.5f, x0 = floorf(xs), fx = xs -
 * x0, columns x0 and x0 + 1 wrapped around the phi seam; ys, y0, fy likewise, rows clamped at the poles; mix(a, b, t) = a * (1 - t) +
 * b * t along x on both rows, then along y, then * scale.  NaN and Inf texels pass through the arithmetic.
 *
 * The table.  sin_row(y) = sinf(3.1415927f * ((float)y + 0.5f) / (float)H); w = ((r * l0 + g * l1) + b * l2) * sin_row(y) with the
 * three luma weights of rt_post_process (csrc/rt_luma.h); a texel is usable where its three channels and w are finite and w > 0;
 * w_max = the largest usable w; q = usable ? 1 + (uint32)(w / w_max * 65534.0f) : 0, so every texel that carries light can be sampled,
 * and the density below is that of the table actually sampled from: quantisation costs variance, never bias.  The table holds, in this
 * order, a header of 24 bytes (u32 width, u32 height, u64 total, f32 w_max, u32 0), the inclusive marginal M[y] = the sum of q over
 * rows 0 .. y (u64, H entries) and the inclusive rows C[y][x] = the sum of q over columns 0 .. x of row y (u32, W * H entries):
 * rt_environment_table_bytes(W, H) = 24 + 8 H + 4 W H.  It is all integers but w_max, a maximum: any scan order gives the same bits.
 * Limits: width <= 16384, height <= 8192, width * height < 2^27 (row sums then fit u32); anything larger is RT_ERR_UNSUPPORTED.
 *
 * The sample.  (record id, sample number s in 0 .. spp - 1) name a texel and a point inside it:
 *     seed_e = film_mix(seed ^ 0xc2b2ae35u)                            a stream of its own, apart from the hemispheres' and the area lights'
 *     u_a    = film_offset(pattern, k, id, seed_e, s, a) + 0.5f        a = 0, 1;  k = the side of a stratified pattern, spp = k * k
 *     a = (double)u_0 * (double)total;  t = min((uint64)a, total - 1);  y = the first row with M[y] > t
 *     fy = min((float)((a - (double)M[y - 1]) / (double)rowsum), 0.99999994f)          rowsum = M[y] - M[y - 1];  M[-1] = 0
 *     b = (double)u_1 * (double)rowsum;  tx = min((uint64)b, rowsum - 1);  x = the first column with C[y][x] > tx
 *     fx = min((float)((b - (double)C[y][x - 1]) / (double)q), 0.99999994f)             q = C[y][x] - C[y][x - 1];  C[y][-1] = 0
 *     (x_f, y_f) = ((float)x + fx, (float)y + fy), dir as above
 *     pdf = (float)((double)q / (double)total) * (float)(W * H) / (19.739209f * sin theta)      per solid angle; sin theta the sample's own
 * pattern, spp and normal_kind have the hemisphere queries' limits and messages.  A table whose header does not name the
 * environment's width and height reads as total = 0; the two searches stay inside the table whatever it holds.
 *
 * Per-entry arrays are sample-major, as the hemisphere queries': entry k = s * n + i, spp * n entries.  The record rules are those of
 * the hit queries.  Every pointer but the descriptor is a device pointer; the descriptor is a small struct read on the host and passed
 * to the kernels by value.  Every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), allocates nothing, uses
 * no workspace beyond the caller's table and may be captured into a HIP graph at once.
 * Checked before any device work, in this order: n >= 2^32 or n * spp >= 2^32 is RT_ERR_UNSUPPORTED; a null scene
 * RT_ERR_INVALID_ARGUMENT (rt_environment_rays, rt_environment_fold); a null descriptor, null texels, a width or height of 0
 * (RT_ERR_INVALID_ARGUMENT), an image over the limits (RT_ERR_UNSUPPORTED), an unknown filter (RT_ERR_INVALID_ARGUMENT); n == 0 is RT_OK
 * and launches nothing; a null required pointer RT_ERR_INVALID_ARGUMENT; then spp, pattern and normal_kind as the hemisphere queries
 * check them; only then is the scene read.
 * Not covered: octahedral or cube maps; mip levels (a lookup takes one or four texels whatever the ray's footprint); the sky inside
 * rt_render_whitted, rt_trace_rays or the distributed pass (the tree loop written from the public calls takes it: trace_rays_levels in
 * Python); Refraction::Infinite rays (the refraction queries hand them back, a caller looks them up itself); rt_multi_* forms; _host
 * forms (rt_environment_*_cpu of include/rt_environment_host.h are the CPU forms).  Multiple importance sampling with the surface's
 * own lobes is the lobe queries' below: rt_environment_pdf returns the density rt_environment_rays divides by. */
#define RT_ENV_NEAREST 0u
#define RT_ENV_BILINEAR 1u
#define RT_ENV_MAX_WIDTH 16384u
#define RT_ENV_MAX_HEIGHT 8192u
typedef struct rt_environment {
    const float *d_texels;  /* height * width * 3 floats, row 0 at the zenith */
    uint32_t width, height;
    float rotation;         /* radians about +y, added to phi */
    float scale;            /* multiplies every looked-up radiance */
    uint32_t filter;        /* RT_ENV_NEAREST or RT_ENV_BILINEAR */
} rt_environment;

/* The radiance along rays that found nothing.  d_rays: n rays, of which the direction is read.  d_count: NULL, or one device u32, the
 * number of live records (a count above n is read as n), as in the tree loop.  d_hits: NULL — every live record is written — or the n
 * hits of the rays: only the records that are "no hit" (kind > 1) are written, the others are left untouched.  The value goes to
 * d_out[3 * d_parent[j] ..], or with d_parent == NULL to d_out[3 * j ..]; n_out is the number of 3-float slots d_out holds, and a
 * slot at or beyond it is not written (0xffffffff, rt_tree_gather's "no candidate", folds nowhere) — rt_tree_fold's addressing.  One
 * kernel, one record per lane, rays read as dwords. */
int rt_environment_lookup(const rt_environment *env, const rt_ray *d_rays, size_t n, const uint32_t *d_count, const rt_hit *d_hits,
                          const uint32_t *d_parent, float *d_out, size_t n_out, void *hip_stream);
/* The sampling table of an environment, built on the device into d_table (rt_environment_table_bytes(width, height) bytes, 8-byte
 * aligned; 0 for an image over the limits): a max reduction, an inclusive scan per row (one workgroup per row) and one over the rows.
 * The luma weights are computed on the host.  Until the last kernel has run the header reads as "no table". */
size_t rt_environment_table_bytes(uint32_t width, uint32_t height);
int rt_environment_table(const rt_environment *env, void *d_table, void *hip_stream);
/* spp directions per hit, drawn from the table.  d_ids: n u32, the record id of the hash, or NULL for id = (uint32_t)i.
 *   d_dirs[3k ..]      dir, for every entry of a record that is a hit while total > 0; zero words otherwise
 *   d_texel[k]         y * W + x of the sampled texel, where d_dirs[k] is written; 0 otherwise (may be NULL)
 *   d_asks[k]          the record is a hit, total > 0, pdf is finite and > 0, and !(dot(dir, N) <= 0) — N by normal_kind, as
 *                      rt_hemisphere_rays chooses it
 *   d_radiance[3k ..]  texel(x, y) * scale / pdf where d_asks[k] — the sampled texel itself, whatever `filter` says; zeros elsewhere
 *   d_rays[k]          rt_hemisphere_rays' shadow ray for that direction: from the hit, face Back, the hit's primitive excluded;
 *                      all-zero words where d_asks[k] is 0 */
int rt_environment_rays(const rt_scene *scene, const rt_environment *env, const void *d_table, const rt_hit *d_hits, size_t n, const uint32_t *d_ids,
                        uint32_t spp, uint32_t pattern, uint32_t seed, uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs,
                        float *d_radiance, uint32_t *d_texel, void *hip_stream);
/* Per record, over the samples s = 0 .. spp - 1 in order: a sample is open where d_asks[k] is set and d_shadow_hits[k] is "no hit" —
 * the light is infinitely far, so whatever the cast found occludes (d_shadow_hits NULL: nothing occludes; it is read only where
 * d_asks[k] is set).  d_diffuse and d_specular are what rt_probe_surfaces returns for d_dirs with n_probes = spp (its probe-major
 * layout is this block's sample-major one).  acc_d = d_diffuse[3k ..] * d_radiance[3k ..] and acc_s = d_specular[3k ..] *
 * d_radiance[3k ..] per channel, the first open sample's as they are and every later one's added; a record without an open sample
 * adds nothing; otherwise D = acc_d / (float)spp, S = acc_s / (float)spp and
 *     rgb = (rgb + D * (1 - shiness)) + S * shiness                     per channel, in place on d_rgb[3i ..]
 * which is rt_area_light_fold's association.  Every operation rounds to f32 and none is fused.  The call ADDS, as that one does; "no
 * hit" records are not written.  d_open: NULL, or spp * n bytes, the flag per sample (0 on a "no hit" record). */
int rt_environment_fold(const rt_scene *scene, const rt_hit *d_hits, size_t n, uint32_t spp, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                        const float *d_radiance, const float *d_diffuse, const float *d_specular, unsigned char *d_open, float *d_rgb,
                        void *hip_stream);

/* ---- material queries: approx, adjust_normal and the Phong terms on caller-supplied hits ------------------------------

 * The material at a hit, which every render and query kernel evaluates between two casts and none of the blocks above returns:
 * Material::approx(hit.at), ColorMaterial::adjust_normal(hit.at.normal) and get_diffuse / get_specular on a MaterialProbe
 * (materials.rs:33-66, 85-103).  rt_material_hits writes them as a record per hit — albedo, shading-normal and object planes for a
 * denoiser or a compositor; transparency, refraction_index and opaque_decay where a generative material makes them depend on uv —
 * and rt_probe_surfaces evaluates the two Phong terms of such records for directions of the caller's own: an area-light sample, an
 * environment direction, a light chosen per record.  (rt_light_terms gives the terms for the lights stored in the scene only, and
 * already multiplied by the light's colour.)  The functions are the ones get_shade runs (csrc/rt_shade.h), with the same operands in
 * the same order, none fused: probe output times light.color is rt_light_terms' diffuse and specular bit for bit.
 * Every pointer is a device pointer unless said otherwise; every call is stream-ordered and asynchronous on hip_stream (NULL = default
 * stream), is one kernel with one record per lane, allocates nothing, uses no workspace and may be captured into a HIP graph at once.
 * Not covered: textures or material functions beyond the enumerated ones; a light colour or attenuation on the probe; rt_multi_* forms. */

typedef struct rt_surface {      /* 18 words, 72 bytes, read and written as dwords */
    float normal[3];             /* ColorMaterial.normal as approx returns it (tangent space) */
    float diffuse_color[3];
    float shiness;
    float specular_color[3];
    float smoothness, transparency, refraction_index, opaque_decay;
    float shading_normal[3];     /* adjust_normal(hit.at.normal), main.rs:410 */
    uint32_t valid;              /* 1: the record was a hit naming a material of the scene */
} rt_surface;

/* main.rs:408-410 per record: d_surfaces[i] = approx(hit.at) of the material d_hits[i].object_index names, and adjust_normal of the
 * hit's normal.  The record rules are the hit queries': a hit whose kind is neither 0 nor 1, or whose object_index >= n_materials, is
 * "no hit" and is written as 18 ZERO WORDS, so the output is defined for every record; a primitive index outside its array does not
 * invalidate (it is not read); NaN and Inf pass through the arithmetic.  The scene's live material array is read: after
 * rt_scene_update_materials the call reports the new material.
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT; n == 0 is RT_OK
 * and launches nothing; a null pointer RT_ERR_INVALID_ARGUMENT. */
int rt_material_hits(const rt_scene *scene, const rt_hit *d_hits, size_t n, rt_surface *d_surfaces, void *hip_stream);
/* The same on HOST arrays: allocates, copies, runs, synchronises the device and copies back. */
int rt_material_hits_host(const rt_scene *scene, const rt_hit *h_hits, size_t n, rt_surface *h_surfaces);

/* materials.rs:46-66 per (probe p, record i), entry k = p * n + i (probe-major, as the light queries are light-major), with
 *     probe = { at.normal: d_surfaces[i].shading_normal, view_direction: d_view[3i ..], light_direction: d_light_dirs[3k ..] }
 *   d_diffuse[3k ..]     get_diffuse(probe):  diffuse_color * cosine where cosine = dot(light_direction, normal) > 0, else +0
 *   d_specular[3k ..]    get_specular(probe): +0 where cosine <= 0, else specular_color * (pow(max(dot(reflected, view_direction), 0),
 *                        1 / (smoothness + EPSILON)) * (that exponent + 8) / (8 pi))
 * d_view holds what the reference puts into view_direction: get_shade passes -hit.ray.direction.  No light colour is applied and
 * nothing is weighted by shiness: the caller multiplies.  Where valid == 0 both are +0.  Only words 3..5, 7..10 and 14..17 of a surface
 * are used.  The call takes NO SCENE: the surface carries everything the probe needs, so a caller may edit it between the two calls —
 * a diffuse_color from a texture of its own, a shading normal from a normal map.
 * Checked before any device work, in this order: n >= 2^32, or n * n_probes >= 2^32, is RT_ERR_UNSUPPORTED; n == 0 or n_probes == 0 is
 * RT_OK and launches nothing; a null pointer RT_ERR_INVALID_ARGUMENT. */
int rt_probe_surfaces(const rt_surface *d_surfaces, size_t n, const float *d_view, const float *d_light_dirs, uint32_t n_probes, float *d_diffuse,
                      float *d_specular, void *hip_stream);
/* The same on HOST arrays. */
int rt_probe_surfaces_host(const rt_surface *h_surfaces, size_t n, const float *h_view, const float *h_light_dirs, uint32_t n_probes,
                           float *h_diffuse, float *h_specular);

/* ---- lobe queries: directions drawn from a surface's own Phong lobes, densities, and the weights that combine two samplers ---------

 * rt_hemisphere_rays draws cosine-distributed directions and rt_environment_rays draws by the sky's brightness; neither looks at the
 * surface's specular lobe, whose exponent reaches 1e5 in the reference scene (smoothness 1e-5): a glossy surface under a sky is black
 * with fireflies, and a small sun over a rough surface is found by the table alone.  This block adds the third sampler, the density
 * of any direction under each sampler, and the weight of multiple importance sampling on the device.  Its fold is
 * rt_environment_fold: there is one weighting convention.  The sequences
 *     one glossy bounce   rt_lobe_rays -> rt_trace_rays(d_rays -> d_radiance, all spp * n of them) -> rt_material_hits +
 *                         rt_probe_surfaces(d_dirs) -> rt_mis_weigh(d_pdf, divide_by_own, no other: d_radiance /= pdf) ->
 *                         rt_environment_fold(d_shadow_hits = NULL)
 *     sky light, both samplers   the environment's samples as in "sky light on hits", with rt_environment_pdf(d_dirs) and
 *                         rt_lobe_pdf(d_dirs) -> rt_mis_weigh(d_radiance, already over its density); the lobe's samples:
 *                         rt_lobe_rays -> rt_cast_rays(d_rays) -> rt_environment_lookup(the casts' misses, into zeros) ->
 *                         rt_environment_pdf(d_dirs) -> rt_mis_weigh(divide_by_own); each set through rt_environment_fold into one rgb
 * are written out in INTEGRATION.md; DESIGN.md §3.33 has what they cost and what f32 does to the sampler at high exponents.
 *
 * The mixture.  With N chosen by normal_kind as the hemisphere queries choose it and V = -d_incoming[i].direction, what get_shade
 * passes as view_direction, in single f32 operations in this order, none fused (csrc/rt_lobe.h, shared by both libraries):
 *     e   = 1 / (smoothness + 1.1920929e-7f)                           get_specular's exponent
 *     R   = (2 * dot(V, N)) * N - V                                    get_specular's `reflected` with V in the place of the light
 *     p_s = shiness > 0 ? (shiness < 1 ? shiness : 1) : 0              NaN reads as 0
 *     pdf(dir) = ((1 - p_s) * max(dot(dir, N), 0)) * 0.31830987f + ((p_s * (e + 1)) * 0.15915494f) * powf(max(dot(dir, R), 0), e)
 * max(x, 0) is x > 0 ? x : 0 and powf is rtdm::powf, skipped for the +0 it would return exactly where get_specular skips it.
 * specular(dir) / pdf(dir) on a surface of shiness 1 is the constant (e + 8) / (4 (e + 1)) times specular_color: that is why the lobe
 * lies about R and not about N.
 *
 * The sample.  u_0 and u_1 are rt_hemisphere_rays' for (id, seed, s) — the same seed_h and the same pattern rules — and
 *     u_2 = film_u(id, film_mix(seed_h ^ 0x27d4eb2fu), s, 0)           never stratified;  lobe = u_2 < p_s
 *     lobe 0   rt_hemisphere_rays' direction about N
 *     lobe 1   c = powf(u_0, 1 / (e + 1));  r = sqrt(max(1 - c * c, 0));  phi = 6.2831855f * u_1
 *              dir = adjust_normal((r * cosf(phi), r * sinf(phi), c), R)
 * and the density written is pdf(dir) above, evaluated at the direction produced, not taken from c.
 *
 * Per-entry arrays are sample-major, entry k = s * n + i.  The record rules are those of the hit queries.  Every pointer but an
 * environment's descriptor is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is
 * one kernel with one record or entry per lane and 256 lanes per workgroup, allocates nothing, uses no workspace and may be captured
 * into a HIP graph at once.
 * Not covered: _host and rt_multi_* forms (rt_*_cpu of include/rt_lobe_host.h are the CPU forms); lobes inside rt_render_*; refraction
 * lobes; any selection probability other than shiness.  More than one bounce is the path queries', below. */
#define RT_MIS_BALANCE 0u /* w = a / (a + b) */
#define RT_MIS_POWER 1u   /* w = a * a / (a * a + b * b) */

/* spp directions per hit from the mixture.  d_ids as rt_hemisphere_rays'; d_incoming[i] is Hit.ray of d_hits[i], as in rt_shade_hits.
 *   d_dirs[3k ..]   dir; zero words for a "no hit" record
 *   d_lobe[k]       1: drawn from the specular lobe; 0: from the diffuse one, or "no hit"
 *   d_pdf[k]        pdf(dir), the mixture's; +0 for a "no hit" record
 *   d_asks[k]       the record is a hit, the pdf is finite and > 0, and !(dot(dir, N) <= 0)
 *   d_rays[k]       rt_hemisphere_rays' shadow ray for dir; all-zero words where d_asks[k] is 0
 * With every shiness 0 the call writes rt_hemisphere_rays' d_rays, d_asks and d_dirs bit for bit (a cosine below 2^-126 * pi, whose
 * density rounds to 0, aside).
 * Checked before any device work as the hemisphere queries check, in their order and with their messages; d_incoming is among the
 * required pointers. */
int rt_lobe_rays(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, const uint32_t *d_ids, uint32_t spp, uint32_t pattern,
                 uint32_t seed, uint32_t normal_kind, rt_ray *d_rays, unsigned char *d_asks, float *d_dirs, float *d_pdf, unsigned char *d_lobe,
                 void *hip_stream);
/* d_pdf[k] = pdf(d_dirs[3k ..]) on d_surfaces[i] with V = d_view[3i ..], k = p * n + i over n_probes directions per record — rt_probe_surfaces'
 * layout and, like it, NO SCENE: N is the record's shading_normal, so normal_kind is RT_HEMISPHERE_SHADING, and RT_HEMISPHERE_GEOMETRIC
 * is refused (a surface record carries no geometric normal).  valid == 0 gives +0.  For rt_material_hits' surfaces and d_view = -d_incoming's
 * direction, the density of rt_lobe_rays' own d_dirs is its d_pdf bit for bit.
 * Checked in this order: n >= 2^32 or n * n_probes >= 2^32 is RT_ERR_UNSUPPORTED; n == 0 or n_probes == 0 is RT_OK and launches nothing; a
 * null pointer, then the normal_kind, RT_ERR_INVALID_ARGUMENT. */
int rt_lobe_pdf(const rt_surface *d_surfaces, size_t n, const float *d_view, const float *d_dirs, uint32_t n_probes, uint32_t normal_kind, float *d_pdf,
                void *hip_stream);
/* The density of `count` directions (3 floats each) under an environment's table: what rt_environment_rays keeps to itself, and what a
 * lobe sample needs when it escapes to the sky.  The direction goes through the lookup's own map to (x_f, y_f) and theta;
 * x = min((uint32)x_f, W - 1), y likewise; q = C[y][x] - C[y][x - 1] and
 *     pdf = (float)((double)q / (double)total) * (float)(W * H) / (19.739209f * sinf(theta))
 * +0 for a zero or non-finite direction, a table whose header names another size, total == 0, and a pdf that is not finite.  d_texel:
 * NULL, or count u32: y * W + x, 0 where no texel is named.  The loads are bounded by the image's size, not by what the table holds.
 * Checked in this order: count >= 2^32 is RT_ERR_UNSUPPORTED; the descriptor as the environment queries check it; count == 0 is RT_OK; a
 * null table, direction or pdf pointer RT_ERR_INVALID_ARGUMENT. */
int rt_environment_pdf(const rt_environment *env, const void *d_table, const float *d_dirs, size_t count, float *d_pdf, uint32_t *d_texel,
                       void *hip_stream);
/* Per entry k of `count`: a = (float)n_own * d_pdf_own[k], b = (float)n_other * d_pdf_other[k], w as the heuristic says.  An a that is
 * not finite or <= 0 gives w = +0.  Otherwise, with d_pdf_other NULL or n_other == 0 there is no other strategy: w = 1, nothing is
 * computed and — without divide_by_own — d_rgb is not touched.
 *   d_weight[k]     w (may be NULL)
 *   d_rgb[3k ..]    *= w, or with divide_by_own *= (w / d_pdf_own[k]); a w of 0 multiplies by +0 either way (may be NULL; not both)
 * Each of a, b, the sum and the quotient rounds to f32 once, so the two strategies' balance weights of one direction sum to 1 within
 * 2^-22.  Checked in this order: count >= 2^32 is RT_ERR_UNSUPPORTED; count == 0 is RT_OK; a null d_pdf_own, or d_weight and d_rgb both
 * NULL, then an unknown heuristic, RT_ERR_INVALID_ARGUMENT. */
int rt_mis_weigh(size_t count, const float *d_pdf_own, uint32_t n_own, const float *d_pdf_other, uint32_t n_other, uint32_t heuristic, int divide_by_own,
                 float *d_weight, float *d_rgb, void *hip_stream);

/* ---- path queries: throughput, Russian roulette and multi-bounce paths on caller-supplied hits ---------------------------------------

 * The lobe queries give one stochastic bounce: rt_lobe_rays draws, rt_trace_rays (the Whitted recursion) answers.  A path tracer written
 * from the public calls takes five launches between two casts — rt_material_hits, rt_lobe_rays, rt_probe_surfaces, rt_mis_weigh and
 * rt_environment_fold — and still has nothing that carries a throughput from bounce to bounce, ends a path by Russian roulette on the
 * device, or averages a pixel's paths.  This block is that inner step as ONE kernel (rt_path_advance), the record it keeps (rt_path),
 * and a begin and a resolve around it.  The loop
 *     rt_path_begin -> [spp copies of the roots' hits and rays]
 *     per bounce b: rt_shade_hits (all slots -> d_emitted) -> rt_environment_lookup (the misses; with a sky) ->
 *                   rt_path_advance(list_b, last = (b == max_bounces)) -> rt_select_records(d_alive -> list_b+1) ->
 *                   rt_cast_rays_indexed(d_next_rays, list_b+1 -> d_hits);  d_incoming = d_next_rays
 *     rt_path_resolve
 * is written out in INTEGRATION.md; DESIGN.md §3.35 has what the fusion saves and the weighting convention.
 *
 * Per-path arrays are sample-major: path k = s * n + i is sample s of root i.  Every pointer is a device pointer; every call is
 * stream-ordered and asynchronous on hip_stream (NULL = default stream), is one kernel with one path or root per lane and 256 lanes per
 * workgroup, allocates nothing, uses no workspace, no atomics, and may be captured into a HIP graph at once.  All arithmetic is
 * csrc/rt_path.h's, single f32 and u32 operations in the order given here, none fused, shared by both libraries.
 * Not covered: refraction lobes inside the step (the "transmission queries" block takes them as a branch beside it); next-event estimation of the sky inside the step (rt_path.pdf is kept for it); _host and rt_multi_*
 * forms (rt_path_*_cpu of include/rt_path_host.h are the CPU forms); paths inside rt_render_*; the inside of the sphere a path leaves
 * (the continuation ray excludes the vertex's primitive for both faces, so a path cannot meet the far, inner side of its own sphere). */
#define RT_PATH_ALIVE 1u     /* the path goes on */
#define RT_PATH_SPECULAR 2u  /* the direction last drawn came from the specular lobe */
#define RT_PATH_ESCAPED 4u   /* ended on a record that is "no hit" */
#define RT_PATH_ROULETTE 8u  /* ended by Russian roulette */
#define RT_PATH_DARK 16u     /* ended: the direction did not ask, or no channel of the new throughput is > 0 (NaN is not) */
typedef struct rt_path {     /* 8 words, 32 bytes, 16-byte aligned: read and written as two 16-byte accesses */
    float beta[3];           /* the throughput */
    float pdf;               /* the density of the direction last drawn; +0 before the first bounce: what a caller's MIS needs on a miss */
    uint32_t root;           /* the root i the path belongs to */
    uint32_t id;             /* the id the counter hash takes: the same for every sample of a root */
    uint32_t bounce;         /* bits 0-23: the bounces taken; bits 24-31: the sample index s, the hash's sample argument */
    uint32_t flags;          /* RT_PATH_ALIVE, with RT_PATH_SPECULAR; or how the path ended; 0: ended by `last` */
} rt_path;

/* spp fresh paths per root: d_paths[k] = { beta 1, pdf +0, root i, id d_ids[i] (NULL: i), bounce s << 24, flags RT_PATH_ALIVE } and
 * d_radiance[3k ..] = 0 for k = s * n + i.  Checked in this order: n >= 2^32 or n * spp >= 2^32 is RT_ERR_UNSUPPORTED; n == 0 is RT_OK and
 * launches nothing; a null d_paths or d_radiance, then spp outside 1 .. 64, then a d_paths that is not 16-byte aligned,
 * RT_ERR_INVALID_ARGUMENT. */
int rt_path_begin(size_t n, uint32_t spp, const uint32_t *d_ids, rt_path *d_paths, float *d_radiance, void *hip_stream);
/* One bounce of the listed paths among m slots.  d_index / d_count are rt_cast_rays_indexed's list: slot j = d_index[e] for
 * e < min(*d_count, m); an index >= m names nothing; a slot is listed at most once.  d_index NULL: every j < m, and d_count is not
 * read.  d_hits[j] is the path's vertex and d_incoming[j] the ray that found it (Hit.ray), as in rt_shade_hits; d_emitted[3j ..] the
 * light the vertex sends back along that ray (rt_shade_hits', the sky's for a miss), or NULL.  For each listed slot whose flags have
 * RT_PATH_ALIVE, in this order:
 *   deposit      d_radiance[3j + c] = d_radiance[3j + c] + beta[c] * d_emitted[3j + c]: the product rounded, then the sum
 *   escape       d_hits[j] is "no hit" by the hit queries' rules: the path ends with RT_PATH_ESCAPED
 *   last         last != 0: the path ends with flags 0 and nothing is drawn
 *   sample       rt_lobe_rays' direction, density, lobe and flag for spp = 1, RT_FILM_UNIFORM, id = path.id and, as the hash's
 *                sample argument, the path's own s (bounce >> 24): the hash's argument carries s, so the seed carries the bounce
 *                alone — seed_b = seed + 0x9e3779b9u * b with b the bounces taken, a u32 wrap; bounce 0 draws with `seed` itself
 *   terms        rt_probe_surfaces' diffuse and specular of that direction on rt_material_hits' surface, V = -d_incoming[j].direction
 *   throughput   t = beta * (1.0f / pdf) per channel — rt_mis_weigh with divide_by_own and no other strategy — and
 *                beta' = (+0 + (diffuse * t) * (1 - shiness)) + (specular * t) * shiness — rt_environment_fold for spp = 1 into a
 *                zeroed rgb, so a -0 reads +0.  The flag is 0, or no channel of beta' is > 0: the path ends with RT_PATH_DARK
 *   roulette     where b + 1 >= rr_start: q = the largest channel of beta' (q = 0, then q = c > q ? c : q for r, g, b: a NaN channel is
 *                passed over), q = q < rr_floor ? rr_floor : q, q = q > 1 ? 1 : q, and
 *                    u_3 = film_u(id, film_mix(seed_h ^ 0x165667b1u), s, 0)
 *                with the sample's seed_h, a stream apart from u_0, u_1 and the lobe's u_2 (0x27d4eb2fu).  u_3 < q: beta' = beta' / q
 *                per channel; else the path ends with RT_PATH_ROULETTE.  rr_start 0xffffffff: no roulette
 *   write        a survivor: beta = beta', pdf, bounce + 1, flags RT_PATH_ALIVE | RT_PATH_SPECULAR as drawn, d_alive[j] = 1 and
 *                d_next_rays[j] = the continuation ray: rt_lobe_rays' shadow ray word for word — origin the vertex's position, the
 *                direction drawn — but for its two face words: face Both, exclusion { hit.kind, hit.index, Both }.  It looks for
 *                the path's next vertex, the nearest surface whichever way it faces; a Back ray is an occlusion query, answered by
 *                back faces only (main.rs:185), and would land on the far, inner side of a closed object and pass an open
 *                surface met from its front.  A path that ended: its flags alone change in the record, d_alive[j] = 0,
 *                d_next_rays[j] all-zero words and d_hits[j] the "no hit" record (kind RT_HIT_NONE, every other word 0), so that
 *                a later rt_shade_hits over all slots spends nothing on it and a later advance cannot revive it
 * Slots that are not listed, and listed ones that are not alive, are not touched.  normal_kind chooses the N the direction is drawn
 * about, as in rt_lobe_rays; the terms take the shading normal.
 * Checked before any device work as rt_lobe_rays checks, in its order and with its messages: m >= 2^32 is RT_ERR_UNSUPPORTED; a null
 * scene; m == 0 is RT_OK and launches nothing; a null pointer (d_index, d_emitted may be NULL; d_count only with d_index); the
 * normal_kind; then an rr_floor outside (0, 1] (NaN is), then a d_paths that is not 16-byte aligned, RT_ERR_INVALID_ARGUMENT. */
int rt_path_advance(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                    const rt_ray *d_incoming, const float *d_emitted, uint32_t seed, uint32_t normal_kind, uint32_t rr_start, float rr_floor, int last,
                    float *d_radiance, rt_ray *d_next_rays, unsigned char *d_alive, void *hip_stream);
/* Per root i of n: the samples s = 0 .. spp - 1 of d_radiance in that order, the first as it is and each later one added, the sum
 * / (float)spp, ADDED to d_rgb[3r ..] with r = d_root[i], or i where d_root is NULL (the caller keeps r inside d_rgb and the r of two
 * roots apart).  No atomics: the same bits on every run.  Checked as rt_path_begin checks: the counts, n == 0, a null d_radiance or
 * d_rgb, spp. */
int rt_path_resolve(const float *d_radiance, size_t n, uint32_t spp, const uint32_t *d_root, float *d_rgb, void *hip_stream);

/* ---- texture queries: mip-mapped image textures and normal maps on caller-supplied hits ------------------------------

 * The reference's GenerativeMaterial takes two closures of uv, diffuse_fn and normal_fn (materials.rs:70-103); rt_material enumerates
 * the three bodies main.rs holds and nothing else, so every rt_hit carries a uv and no surface can show an image.  This block is an
 * approx() whose diffuse_fn / normal_fn read an image, followed by the unchanged adjust_normal: rt_texture_surfaces edits the
 * rt_surface records rt_material_hits wrote, and rt_light_terms_surfaces is rt_light_terms with the material and the shading normal
 * taken from those records, so that an edited surface reaches get_shade's own lights as it reaches rt_probe_surfaces.  The sequence
 *     rt_material_hits -> [rt_texture_footprint ->] rt_texture_surfaces per texture binding -> rt_light_rays -> casts ->
 *     rt_light_terms_surfaces -> rt_light_fold
 * is written out in INTEGRATION.md; DESIGN.md §3.34 has what the calls cost.
 *
 * The texture.  A pyramid of row-major levels of 3 floats per texel (linear RGB, or a tangent-space vector), level 0 first, level l of
 * extent max(1, width >> l) by max(1, height >> l); a full pyramid has rt_texture_levels(w, h) = 1 + floor(log2(max(w, h))) levels.
 * The caller owns the memory and fills level 0; rt_texture_pyramid makes the others.  uv maps to the point p = uv * scale + offset and,
 * on a level of extent (w, h), to the texel-space coordinate s = p * (float)extent per axis.  All arithmetic is csrc/rt_texture.h's,
 * single f32 and u32 operations in the order given here, none fused, shared by both libraries.
 *
 * Every device pointer is stream-ordered and asynchronous on hip_stream (NULL = default stream); no call allocates or uses a workspace
 * and each may be captured into a HIP graph at once.  A descriptor is read on the host, at the call.
 * Not covered: sRGB or 8-bit texels; anisotropic filtering; mirror wrap; specular, shiness or transparency maps; textures inside
 * rt_render_*, rt_trace_rays or the distributed pass; _host and rt_multi_* forms (rt_*_cpu of include/rt_texture_host.h are the CPU
 * forms); mip levels for the environment. */
#define RT_TEX_NEAREST 0u
#define RT_TEX_BILINEAR 1u
#define RT_TEX_TRILINEAR 2u
#define RT_TEX_REPEAT 0u
#define RT_TEX_CLAMP 1u
#define RT_TEX_MAX_SIDE 16384u
#define RT_TEX_MODULATE 1u            /* rt_texture_surfaces: diffuse_color *= sample, not = sample */
#define RT_TEX_NORMALIZE 2u           /* rt_texture_surfaces: normal = v / |v| */
#define RT_TEX_ALL_OBJECTS 0xffffffffu
typedef struct rt_texture {
    const float *d_texels;  /* the whole pyramid: rt_texture_pyramid_floats(width, height, n_levels) floats */
    uint32_t width, height; /* of level 0: 1 .. RT_TEX_MAX_SIDE each */
    uint32_t n_levels;      /* 1 .. rt_texture_levels(width, height); 1: level 0 only */
    uint32_t filter;        /* RT_TEX_NEAREST, RT_TEX_BILINEAR, RT_TEX_TRILINEAR */
    uint32_t wrap_u, wrap_v; /* RT_TEX_REPEAT, RT_TEX_CLAMP */
    float scale[2], offset[2];
} rt_texture;               /* 48 bytes */

/* 1 + floor(log2(max(width, height))); 0 for a side of 0.  Host arithmetic. */
uint32_t rt_texture_levels(uint32_t width, uint32_t height);
/* The floats of levels 0 .. n_levels - 1: 3 * sum of the extents' products; 0 for a side of 0 or above RT_TEX_MAX_SIDE, n_levels 0 or
 * above rt_texture_levels.  Host arithmetic. */
size_t rt_texture_pyramid_floats(uint32_t width, uint32_t height, uint32_t n_levels);

/* Levels 1 .. n_levels - 1 from level 0, in place in tex->d_texels: the exact box filter for any extent, x before y.  Along an axis of
 * the source level, destination texel x of a source p(0 ..):
 *     extent 1         p(0)
 *     extent 2m        (p(2x) + p(2x + 1)) * 0.5f
 *     extent 2m + 1    (((float)(m - x) * p(2x) + (float)m * p(2x + 1)) + (float)(1 + x) * p(2x + 2)) / (float)(2m + 1)
 * The three integer weights are what of each source texel lies under the destination texel: no column is dropped.  The rows a
 * destination texel covers are reduced along x first, then those up to three partial rows along y by the same rule.  One launch per
 * level while the source level is above 32 texels either way; from the first level whose source is at most 32 x 32, one workgroup
 * makes all the remaining levels in one launch through LDS.  Each level is computed from the f32 values of the one before, so both
 * forms give the same bits.  A texel that is not finite spreads by the arithmetic.
 * Checked before any device work, in this order: a null texture or null texels, a side of 0 — RT_ERR_INVALID_ARGUMENT; a side above
 * RT_TEX_MAX_SIDE — RT_ERR_UNSUPPORTED; n_levels, filter, wrap — RT_ERR_INVALID_ARGUMENT.  n_levels == 1 launches nothing. */
int rt_texture_pyramid(const rt_texture *tex, void *hip_stream);

/* The uv-space length a ray cone covers at each hit; it depends on no texture.  d_incoming[i] is Hit.ray of d_hits[i].
 *     w = width0 + spread * magnitude(hit.position - ray.origin)         width0 = d_width0[i], or 0 with d_width0 NULL
 *     c = max(|dot(D / |D|, hit.normal)|, 2^-6)                          D = ray.direction
 *     ratio = sqrt(|du1 * dv2 - du2 * dv1| / magnitude(cross(e1, e2)))   a triangle: e_k = v_k.position - v_0.position, du_k and dv_k
 *                                                                        likewise, of the scene's live vertices
 *             0.28209479f / radius                                       a sphere
 *     d_footprint[i] = w * ratio / c
 * +0 — which selects level 0 — for a "no hit" record (the hit queries' rules), a primitive index outside its array, a primitive
 * without area (a cross product of length 0, or not finite; a radius that is not finite and > 0), and any result that is not finite.
 * Nothing is indexed with a word that was not checked against its array.  After rt_scene_update_vertices the new vertices are read.
 * Checked in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT; n == 0 is RT_OK; a null hit,
 * incoming-ray or footprint pointer RT_ERR_INVALID_ARGUMENT. */
int rt_texture_footprint(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, float spread, const float *d_width0,
                         float *d_footprint, void *hip_stream);

/* The filtered lookup.  Record i reads (u, v) = d_uv[i * uv_stride_words ..] and writes 3 floats at d_out[i * out_stride_words ..]:
 * with d_uv = (const float *)d_hits + 9 and a stride of 13 the uv is read inside rt_hit records, and the result may go into any
 * field of a record without a copy.  d_footprint: n floats or NULL for 0.
 *   RT_TEX_NEAREST    x = min((uint32)x_f, W - 1), x_f = s wrapped by s - floorf(s / W) * W (RT_TEX_REPEAT) or left as it is
 *                     (RT_TEX_CLAMP), then clamped to [0, W]; y likewise
 *   RT_TEX_BILINEAR   texel centres at + 0.5: xs = x_f - 0.5f, x0 = floorf(xs), fx = xs - x0, texels x0 and x0 + 1 wrapped or clamped;
 *                     a * (1 - fx) + b * fx along x on both rows, then the same along y — rt_environment_lookup's mixing
 *   RT_TEX_TRILINEAR  t = footprint * max(|scale_u| * W, |scale_v| * H); !(t > 1): level 0, bilinear; else l = the unbiased exponent
 *                     of t and f = t * 2^-l - 1, both exact; the bilinear samples of levels l and l + 1 mixed by f; with l at or
 *                     above the top level, that level alone.  No transcendental is evaluated.
 * The other two filters read level 0 and no footprint.  A u or v that is not finite writes zeros.
 * Checked in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; the descriptor as rt_texture_pyramid checks it; n == 0 is RT_OK; a null uv
 * or output pointer, then uv_stride_words < 2 or out_stride_words < 3, RT_ERR_INVALID_ARGUMENT. */
int rt_texture_sample(const rt_texture *tex, const float *d_uv, size_t uv_stride_words, const float *d_footprint, size_t n, float *d_out,
                      size_t out_stride_words, void *hip_stream);

/* rt_surface records edited in place: approx() with diffuse_fn / normal_fn read from images.  Record i is edited only where
 * d_surfaces[i].valid != 0, d_hits[i].object_index == object_index (RT_TEX_ALL_OBJECTS: any) and the hit's uv is finite.
 *   diffuse_tex   diffuse_color = sample(uv); with RT_TEX_MODULATE the old colour times the sample
 *   normal_tex    normal = sample(uv); with RT_TEX_NORMALIZE v / magnitude(v), and a length that is 0 or not finite leaves normal and
 *                 shading_normal as they are; shading_normal = adjust_normal(normal, hit.normal), csrc/rt_shade.h's function called
 *                 as rt_material_hits calls it
 * Either texture may be NULL (both: nothing is launched).  Words 0..5 and 14..16 of an edited record move and no other.
 * Checked in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; each descriptor given; n == 0 is RT_OK; a null hit or surface pointer, then
 * unknown flags, RT_ERR_INVALID_ARGUMENT. */
int rt_texture_surfaces(const rt_texture *diffuse_tex, const rt_texture *normal_tex, const rt_hit *d_hits, const float *d_footprint, size_t n,
                        uint32_t object_index, uint32_t flags, rt_surface *d_surfaces, void *hip_stream);

/* rt_light_terms with the material (words 0..13 of the record, Material::approx's fields in its order; get_diffuse and get_specular
 * consume words 3..5 and 7..10) and the shading normal (words 14..16) taken from d_surfaces[i] instead of the scene's material; a record
 * whose valid is 0 is "no hit".  The position, the occlusion rule, approximate_into_directional,
 * get_diffuse, get_specular and the wave-level skip are rt_light_terms': on the records rt_material_hits wrote, unedited, d_lit,
 * d_diffuse and d_specular are that call's bit for bit.  rt_light_fold stays the fold: a texture does not change shiness.
 * Checked as rt_light_terms checks, with the surfaces among the pointers. */
int rt_light_terms_surfaces(const rt_scene *scene, const rt_surface *d_surfaces, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n,
                            uint32_t light_first, uint32_t light_count, const unsigned char *d_asks, const rt_hit *d_shadow_hits,
                            unsigned char *d_lit, float *d_diffuse, float *d_specular, void *hip_stream);

/* ---- refraction queries: get_refract bounce by bounce on caller-supplied hits ------------------------------

 * get_refract (main.rs:343-405) opened into the calls between its casts.  rt_refract_rays runs the whole walk through the glass in one
 * kernel, its 1 to 11 casts inside; here every one of those casts is a record like every other ray, so that a caller can touch the walk
 * — a bounce limit of its own, an absorption rule per segment, a stop at the first interior hit — and so that the casts go through
 * rt_select_records + rt_cast_rays_indexed, which on a scene walked breadth-first take that walk.  The sequence
 *     rt_refract_enter, then eleven times:
 *     rt_select_records(d_flags) -> rt_cast_rays_indexed(d_rays -> d_inside_hits, d_ray_count) -> rt_refract_step
 * on a d_escape zeroed once up front gives rt_refract_rays' kind, escape ray and cast count bit for bit, and its travel where the record
 * escaped (INTEGRATION.md writes it out; DESIGN.md §3.15 says why the bits are the same).  Fewer rounds leave the unfinished records
 * RT_REFR_WALKING with their state complete: later rounds continue them.  Records are the hit queries': entry i of d_incoming is Hit.ray
 * of d_hits[i]; every pointer is a device pointer and all are required; every call is stream-ordered and asynchronous on hip_stream
 * (NULL = default stream), is one kernel with one record per lane (any n below 2^32 in one launch), uses no workspace and may be
 * captured into a HIP graph at once.
 * The state of a walk is five caller-owned arrays of n entries, written by rt_refract_enter and advanced by rt_refract_step:
 *   d_kind[i]    RT_REFR_WALKING while the walk goes on; then 0 Escaped, 1 Infinite, 2 Trapped, or RT_HIT_NONE (no hit), as rt_refract_rays
 *   d_rays[i]    the ray to cast next while walking; the ray whose cast missed when Infinite (Refraction::Infinite's ray, main.rs:154-156)
 *   d_travel[i]  the running travel_distance: the sum so far while walking, rt_refract_rays' travel when Escaped.  For Infinite and Trapped
 *                it stays as computed — rt_refract_rays reports 0 there; a caller that wants that writes it
 *   d_casts[i]   the casts answered for the record so far, a miss included: the per-record cast count; its sum over the records is what
 *                rt_cast_rays_indexed added to d_ray_count
 *   d_flags[i]   1 exactly where d_rays[i] is to be cast next: the operand of rt_select_records
 * The record rules are those of the hit-query block: a hit whose kind is neither 0 nor 1, or whose object_index >= n_materials, is "no
 * hit"; a primitive index outside its array only ever serves as an exclusion; a face above 1 reads as Back; NaN and Inf pass through the
 * arithmetic.  The state is the caller's as well and is validated, never trusted: a d_kind word other than RT_REFR_WALKING is "finished"
 * whatever it holds; d_casts only enters the test `casts < 10` (10, 2^31 or any other value at or above 10 fails it); nothing is indexed
 * with a state word; d_rays and d_inside_hits are read as rt_cast_rays reads a ray and as the hit queries read a hit (an inside hit whose
 * kind is neither 0 nor 1 is a miss; an exclusion index beyond its array excludes nothing).
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene RT_ERR_INVALID_ARGUMENT; n == 0 is RT_OK
 * and launches nothing; a null pointer RT_ERR_INVALID_ARGUMENT.
 * Not covered: _host forms (the calls sit between device calls); rt_multi_* forms. */

#define RT_REFR_WALKING 3u /* beside 0 Escaped, 1 Infinite, 2 Trapped and RT_HIT_NONE */

/* main.rs:354-368 per record, with k = approx(hit.at).refraction_index:
 *   a record that is "no hit"                     d_kind RT_HIT_NONE, an all-zero d_rays[i], d_flags 0
 *   refract(hit.normal, hit.ray.direction, k) None  d_kind 2 (Trapped, main.rs:356-358), an all-zero d_rays[i], d_flags 0
 *   otherwise                                     d_kind RT_REFR_WALKING, d_flags 1 and d_rays[i] = ray_inside: origin = the hit's position,
 *                                                 direction = refract_in normalised a second time, face Back, exclusion { hit.kind,
 *                                                 hit.index, Front } — bit for bit the ray rt_refract_rays casts first
 * and for every record d_travel[i] = +0 and d_casts[i] = 0. */
int rt_refract_enter(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_ray *d_rays, uint32_t *d_kind,
                     float *d_travel, uint32_t *d_casts, unsigned char *d_flags, void *hip_stream);
/* main.rs:371-402 for ONE answered cast.  A record whose d_kind[i] is not RT_REFR_WALKING is finished: d_flags[i] = 0 and nothing else is
 * written (so d_escape[i] of a record rt_refract_enter finished is never written: zero d_escape once, before the first round).  For a
 * walking record d_inside_hits[i] is what a cast of d_rays[i] wrote (hit_inside); with j = d_casts[i] and k of the material of d_hits[i]:
 *   d_casts[i] = j + 1
 *   hit_inside is a miss          d_kind 1 (Infinite); d_rays[i] and d_travel[i] stay as they are
 *   otherwise                     travel = distance(hit_inside.position, hit.position) when j == 0 (main.rs:375), else
 *                                 travel = d_travel[i] + distance(origin of d_rays[i], hit_inside.position) (main.rs:385); d_travel[i] = travel;
 *                                 out = refract(hit_inside.normal, direction of d_rays[i], 1 / k), and then
 *     out is None && travel <= max_distance && j < 10 (in that order, main.rs:378)
 *                                 d_rays[i] = get_reflect(&hit_inside): origin hit_inside.position, the reflected direction, face Back,
 *                                 exclusion { hit_inside.kind, hit_inside.index, invert(hit_inside.face_direction) }; d_flags[i] = 1; the
 *                                 kind stays RT_REFR_WALKING and d_escape[i] is not written
 *     out is Some                 d_kind 0 (Escaped); d_escape[i] = escape_ray as rt_refract_rays writes it: origin hit_inside.position,
 *                                 direction out normalised again, face Front, exclusion { hit_inside.kind, hit_inside.index, Back }
 *     anything else               d_kind 2 (Trapped)
 * Where the walk ends without an escape ray (Infinite, Trapped) d_escape[i] is all-zero words; where it ends, d_flags[i] = 0.
 * max_distance: the reference passes 100.0. */
int rt_refract_step(const rt_scene *scene, const rt_hit *d_hits, size_t n, float max_distance, const rt_hit *d_inside_hits, rt_ray *d_rays,
                    uint32_t *d_kind, float *d_travel, uint32_t *d_casts, unsigned char *d_flags, rt_ray *d_escape, void *hip_stream);

/* ---- transmission queries: paths that pass through glass ------------------------------------------------------------------------------

 * The path queries treat every surface as its two Phong lobes; ray_trace (main.rs:502-514) and distributed_ray_trace (main.rs:595-611)
 * send light through a material with transparency > 0.  The refraction queries above open that walk into its casts.  What no caller can
 * supply from the existing calls is the stochastic choice per vertex between "through the glass" and "off the lobes", and the step that
 * folds a finished walk into the 32-byte rt_path record.  These two calls are that, and bounce b of the path loop becomes
 *     rt_shade_hits -> rt_environment_lookup (with a sky) -> rt_path_branch(list_b, last) ->
 *     rt_select_records(d_lobe) -> rt_path_advance(that list) ->
 *     walk_rounds times: rt_select_records(d_walk_flags) -> rt_cast_rays_indexed(d_walk_rays -> d_inside_hits) -> rt_refract_step (all m) ->
 *     rt_select_records(d_transmit) -> rt_path_transmit(that list) ->
 *     rt_select_records(d_alive -> list_b+1) -> rt_cast_rays_indexed(d_next_rays, list_b+1 -> d_hits)
 * (INTEGRATION.md writes it out; DESIGN.md §3.36 has the estimator and what the calls cost.)
 *
 * The estimator.  The Whitted weights at a vertex are (1 - t) for shade + lobes and t for the refraction, t = approx(hit.at).transparency
 * (main.rs:480-502).  A path takes the refraction with probability t and the lobes with probability 1 - t: either way the weight over the
 * probability is 1, and beta is not touched by the choice.  A path that takes the lobes goes through rt_path_advance unchanged, deposit
 * included.  A path that takes the refraction deposits nothing at this vertex (the (1 - t) share of the direct light is the lobe paths'
 * deposit), walks get_refract, has beta multiplied by opaque_decay.powf(travel_distance) (main.rs:508) where the walk Escaped, and goes
 * on along the escape ray; a transmission counts as one bounce however many casts the walk took.
 *
 * Every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is one kernel
 * with one listed slot per lane and 256 lanes per workgroup, allocates nothing, uses no workspace, no atomics, and may be captured into a
 * HIP graph at once.  The list is rt_path_advance's: slot j = d_index[e] for e < min(*d_count, m); an index >= m names nothing; d_index
 * NULL: every j < m, and d_count is not read.  Records are read by the hit queries' rules.  The walk's state words are the caller's and
 * are validated, never trusted, by the refraction block's rule: a d_kind word is compared, and nothing is indexed with a state word.
 * All arithmetic is csrc/rt_transmit.h's, single f32 and u32 operations in the order given here, none fused, shared by both libraries.
 * Checked before any device work, in rt_path_advance's order and with its messages: m >= 2^32 is RT_ERR_UNSUPPORTED; a null scene; m == 0
 * is RT_OK and launches nothing; a null pointer (d_index may be NULL; d_count only with d_index); (rt_path_transmit) an rr_floor outside
 * (0, 1]; then a d_paths that is not 16-byte aligned, RT_ERR_INVALID_ARGUMENT.
 * Not covered: rough transmission — the event is a delta: no roughness, and no scatter_hit perturbation of the incoming direction;
 * _host and rt_multi_* forms (rt_path_branch_cpu and rt_path_transmit_cpu of include/rt_transmit_host.h are the CPU forms); paths inside
 * rt_render_*. */
#define RT_PATH_TRANSMITTED 32u /* with RT_PATH_ALIVE: the path's last event was a transmission (never with RT_PATH_SPECULAR) */
#define RT_PATH_TRAPPED 64u     /* ended: the walk through the glass did not escape (Infinite, Trapped, no hit, or left RT_REFR_WALKING) */

/* The choice, per listed slot whose flags have RT_PATH_ALIVE.  With b the bounces taken, s the sample index (bounce >> 24) and seed_h the
 * hemisphere seed of seed + 0x9e3779b9u * b — exactly rt_path_advance's —
 *     u_4 = film_u(id, film_mix(seed_h ^ 0x85ebca6bu), s, 0)
 * a fifth stream, beside u_0, u_1, the lobe's u_2 (0x27d4eb2fu) and the roulette's u_3 (0x165667b1u).  The path transmits iff d_hits[j] is
 * a hit and u_4 < transparency of approx(hit.at): film_u lies in [0, 1), so t = 0 never transmits, t >= 1 always does and a NaN t never
 * does; a "no hit" record takes the lobes, so that rt_path_advance ends it with RT_PATH_ESCAPED and deposits its sky.
 *   a path that transmits, last == 0   d_lobe[j] = 0, d_transmit[j] = 1, and d_walk_rays[j], d_kind[j], d_travel[j], d_casts[j] and
 *                                      d_walk_flags[j] are what rt_refract_enter writes for d_hits[j] and d_incoming[j], bit for bit
 *                                      (RT_REFR_WALKING with ray_inside and flag 1, or 2 Trapped at entry with an all-zero ray and flag 0)
 *   a path that transmits, last != 0   the path ends here: flags 0 (they alone change in the record), d_lobe[j] = d_transmit[j] = 0,
 *                                      nothing walks, and d_hits[j] becomes the "no hit" record, as rt_path_advance leaves an ended path
 *   a path that takes the lobes        d_lobe[j] = 1, d_transmit[j] = 0
 *   a listed slot that is not alive    d_lobe[j] = d_transmit[j] = 0
 * Every listed slot that does not walk gets the state of a finished walk: d_kind[j] = RT_HIT_NONE, d_walk_flags[j] = 0, an all-zero
 * d_walk_rays[j], d_travel[j] = +0 and d_casts[j] = 0, so that a later rt_refract_step over all m slots skips it.  Slots that are not
 * listed are not touched.  d_paths is read (and for a path `last` ends, written) as the 16-byte second half of the record. */
int rt_path_branch(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                   const rt_ray *d_incoming, uint32_t seed, int last, unsigned char *d_lobe, unsigned char *d_transmit, rt_ray *d_walk_rays,
                   uint32_t *d_kind, float *d_travel, uint32_t *d_casts, unsigned char *d_walk_flags, void *hip_stream);
/* The fold of a finished walk, per listed slot whose flags have RT_PATH_ALIVE, with d_kind[j], d_travel[j] and d_escape[j] as
 * rt_refract_step left them and d_hits[j] still the vertex the path entered the glass at:
 *   d_kind[j] is 0 (Escaped) and d_hits[j] is a hit
 *                w = powf(opaque_decay of approx(hit.at), d_travel[j]) — the function of main.rs:508 in the Whitted kernels — and
 *                beta' = beta * w per channel; then rt_path_advance's own tail: no channel of beta' is > 0 (NaN is not): the path ends
 *                with RT_PATH_DARK; where b + 1 >= rr_start its roulette with the same u_3 (this path did not use u_3 at this bounce):
 *                RT_PATH_ROULETTE, or beta' = beta' / q
 *   anything else (1 Infinite, 2 Trapped, RT_HIT_NONE, a walk still RT_REFR_WALKING because the caller ran fewer rounds, any other word)
 *                the path ends with RT_PATH_TRAPPED
 *   write        a survivor: beta = beta', pdf = +0 (a delta event that no other strategy could have drawn, as before the first
 *                bounce), bounce + 1, flags RT_PATH_ALIVE | RT_PATH_TRANSMITTED, d_alive[j] = 1 and d_next_rays[j] = d_escape[j].  A path
 *                that ended: what rt_path_advance writes — its flags alone change in the record, d_alive[j] = 0, d_next_rays[j] all-zero
 *                words and d_hits[j] the "no hit" record
 * and for every listed slot, alive or not, d_kind[j] = RT_HIT_NONE and d_walk_flags[j] = 0: stale walk state never walks in a later
 * bounce.  Slots that are not listed are not touched; of a listed slot that is not alive nothing else is. */
int rt_path_transmit(const rt_scene *scene, rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, rt_hit *d_hits,
                     uint32_t *d_kind, const float *d_travel, const rt_ray *d_escape, uint32_t seed, uint32_t rr_start, float rr_floor,
                     rt_ray *d_next_rays, unsigned char *d_alive, unsigned char *d_walk_flags, void *hip_stream);

/* ---- connection queries: next-event estimation of the sky in path loops --------------------------------------------------------------

 * The path loop finds the scene's lights at every vertex (rt_shade_hits) and the sky only when a lobe-sampled ray happens to leave the
 * scene, where rt_environment_lookup deposits it unweighed: under a sky with a small bright sun that estimator is noisy.  The lobe
 * queries' "sky light, both samplers" has the cure for one bounce in seven to eight launches and carries no throughput.  These three
 * calls are what a caller could not supply from outside — a sky sample per vertex from the path's own hash streams, the throughput
 * multiplied in before the shadow cast is answered, and the escape weighed by the density rt_path_advance stored in the record — and
 * bounce b of the path loop becomes
 *     rt_shade_hits -> rt_environment_lookup -> rt_path_weigh_escape(list_b) ->
 *     rt_path_connect(list_b, last) -> rt_path_advance(list_b, last) ->                                 [b < max_bounces, from here on]
 *     rt_select_records(d_asks -> the asking list) -> rt_cast_rays_indexed(d_shadow_rays, that list -> d_shadow_hits) ->
 *     rt_path_settle(that list) ->
 *     rt_select_records(d_alive -> list_b+1) -> rt_cast_rays_indexed(d_next_rays, list_b+1 -> d_hits)
 * With the transmission queries rt_path_branch and rt_select_records(d_lobe) come first and rt_path_connect and rt_path_advance take that
 * list: a path that goes through the glass deposits nothing at the vertex and connects nothing there.  rt_path_connect precedes
 * rt_path_advance, which advances beta and rewrites the hit of a path that ends; rt_path_settle follows its deposit, so the order of the
 * additions into d_radiance is fixed: deposit, then connection.  On the last bounce the connection and the settlement are left out (with
 * `last` the call asks nothing), so both estimators integrate the same set of paths.  INTEGRATION.md writes the sequence out; DESIGN.md
 * §3.37 has the estimator, the bytes and the resources.
 *
 * The estimator.  At a vertex two strategies can find the sky along a direction d: the connection, which draws d from the table with
 * density p_env(d) = rt_environment_pdf's, and the next lobe sample, density p_lobe(d) = rt_lobe_pdf's about the sampling normal.  Each
 * is weighed by rt_mis_weigh's weight against the other, one sample each; the weights add up to 1 wherever either density is positive.
 * The sky a path sees after a delta event — a camera ray, a ray that left glass: pdf +0 in the record — no connection could have found:
 * it keeps its full weight.  A connection is occluded by whatever its shadow ray hits, glass included, so light that reaches a vertex
 * through glass is counted by the transmitted path alone.  The connection's radiance is the sampled texel's and the escape's is
 * rt_environment_lookup's: with RT_ENV_NEAREST the two estimate one integrand.
 *
 * The streams.  With b the bounces taken, s the sample index (bounce >> 24) and seed_b = seed + 0x9e3779b9u * b — rt_path_advance's —
 * the connection's two uniforms are rt_environment_rays' for seed_b, id and s: film_mix(seed_b ^ 0xc2b2ae35u) is their stream, while the
 * lobe's u_0 and u_1 come from film_mix(seed_b ^ 0x85ebca6bu).  The two directions of a vertex are drawn independently.
 *
 * Every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream), is one kernel
 * with one listed slot per lane and 256 lanes per workgroup, allocates nothing, uses no workspace, no atomics, and may be captured into a
 * HIP graph at once.  The list is rt_path_advance's: slot j = d_index[e] for e < min(*d_count, m); an index >= m names nothing; d_index
 * NULL: every j < m, and d_count is not read.  Slots that are not listed are not touched.  d_paths is read as two 16-byte accesses and
 * never written.  d_table is rt_environment_table's for this env; one whose header names another size reads as a table without light,
 * as in rt_environment_pdf, and nothing is read outside the size the descriptor gives.  All arithmetic is csrc/rt_connect.h's, single f32
 * and u32 operations in the order given here, none fused, shared by both libraries.
 * Checked before any device work, in rt_path_advance's order and with its messages: m >= 2^32 is RT_ERR_UNSUPPORTED; a null scene
 * (rt_path_connect); the descriptor, as rt_environment_rays checks it; m == 0 is RT_OK and launches nothing; a null pointer (d_index may
 * be NULL; d_count only with d_index; d_shadow_hits may be NULL); the normal_kind (rt_path_connect), then an unknown heuristic; then a
 * d_paths that is not 16-byte aligned or a d_table that is not 8-byte aligned, RT_ERR_INVALID_ARGUMENT.
 * Not covered: connections to the scene's own lights with a radius (area-light next-event estimation inside the loop); more than one
 * sky sample per vertex; connections through glass; _host and rt_multi_* forms (rt_path_connect_cpu, rt_path_settle_cpu and
 * rt_path_weigh_escape_cpu of include/rt_connect_host.h are the CPU forms); paths inside rt_render_*; any change to rt_path_advance's
 * record or bits. */

/* The connection, per listed slot whose flags have RT_PATH_ALIVE, with d_hits[j] the path's vertex and d_incoming[j] the ray that found
 * it, before rt_path_advance moves the path.  `last`, a vertex that is "no hit" by the hit queries' rules and a table without light ask
 * nothing and draw nothing.  Otherwise, in this order:
 *   sample     rt_environment_rays' direction, texel and density for spp = 1, RT_FILM_UNIFORM, id = path.id, sample s and seed_b;
 *              r = texel * scale / pdf where that call asks (a finite density > 0, a direction that leaves the surface about the
 *              normal normal_kind chooses)
 *   densities  p_env = rt_environment_pdf(direction); p_lobe = rt_lobe_pdf(direction) on the surface rt_path_advance samples: the
 *              normal of normal_kind, V = -d_incoming[j].direction, the material's shiness and smoothness
 *   weight     w = rt_mis_weigh's for n_own = n_other = 1, p_env against p_lobe, and r = r * w per channel
 *   throughput t = beta * r per channel
 *   terms      rt_probe_surfaces' diffuse and specular of the direction on rt_material_hits' surface, and
 *              pending = (+0 + (diffuse * t) * (1 - shiness)) + (specular * t) * shiness — rt_environment_fold for spp = 1 into a
 *              zeroed rgb, so a -0 reads +0
 * The slot asks where rt_environment_rays asks and w is finite.  d_asks[j] = 1 or 0; d_shadow_rays[j] = rt_hemisphere_rays' ray along
 * the direction where it asks, all-zero words where it does not; d_pending[3j ..] is written where it asks and left as it is elsewhere.
 * Listed slots that are not alive are not touched. */
int rt_path_connect(const rt_scene *scene, const rt_environment *env, const void *d_table, const rt_path *d_paths, size_t m, const uint32_t *d_index,
                    const uint32_t *d_count, const rt_hit *d_hits, const rt_ray *d_incoming, uint32_t seed, uint32_t normal_kind, uint32_t heuristic,
                    int last, rt_ray *d_shadow_rays, unsigned char *d_asks, float *d_pending, void *hip_stream);
/* The settlement, per listed slot, alive or not (rt_path_advance may have ended the path since it connected): where d_asks[j] != 0 and
 * d_shadow_hits[j] is "no hit" at all (kind word > 1: rt_environment_fold's rule; d_shadow_hits NULL: nothing occludes),
 * d_radiance[3j + c] = d_radiance[3j + c] + d_pending[3j + c]; either way d_asks[j] = 0, so that the flags of all m slots are 0 again
 * when the next bounce connects.  d_paths is not read: it is taken so that the three calls share their list arguments and checks. */
int rt_path_settle(const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, unsigned char *d_asks, const rt_hit *d_shadow_hits,
                   const float *d_pending, float *d_radiance, void *hip_stream);
/* The escape, per listed slot whose flags have RT_PATH_ALIVE, after rt_shade_hits and rt_environment_lookup filled d_emitted and before
 * rt_path_advance deposits it: where d_hits[j] is "no hit" by rt_environment_lookup's rule (kind word > 1 — rt_shade_hits wrote zeros
 * there, so d_emitted[3j ..] is the sky alone), the record's pdf is finite and > 0 and the table has light,
 *     d_emitted[3j + c] = d_emitted[3j + c] * w,  w = rt_mis_weigh's for n_own = n_other = 1, pdf against
 *                                                     rt_environment_pdf(d_incoming[j].direction)
 * A pdf of +0 (a camera ray, a ray that left glass), a hit, a slot that is not alive and a table without light leave d_emitted alone. */
int rt_path_weigh_escape(const rt_environment *env, const void *d_table, const rt_path *d_paths, size_t m, const uint32_t *d_index,
                         const uint32_t *d_count, const rt_hit *d_hits, const rt_ray *d_incoming, uint32_t heuristic, float *d_emitted, void *hip_stream);

/* ---- light-connection queries: one sampled scene light per path vertex ------------------------------------------------------------

 * The path loop lights every vertex with rt_shade_hits, which evaluates all of the scene's lights as points: one shadow cast per light
 * and vertex, and a hard edge on every shadow inside a path-traced frame.  These two calls are next-event estimation of the scene's own
 * lights — what a caller could not put together from rt_area_light_rays, rt_light_terms and the connection queries from outside: the
 * light and the point on it drawn from the path's own hash streams, the throughput multiplied in before rt_path_advance moves it, and
 * get_shade's occlusion rule applied after rt_path_advance has rewritten the hit of a path that ended.  One light per vertex, one shadow
 * cast per vertex, soft shadows where the lights have radii.  Bounce b of the path loop becomes
 *     [rt_shade_hits is left out: d_emitted of the hits is zeros] -> rt_environment_lookup (the sky on the misses, if any) ->
 *     rt_path_connect_lights(list_b) -> rt_path_advance(list_b, last) ->
 *     rt_select_records(d_asks -> the asking list) -> rt_cast_rays_indexed(d_shadow_rays, that list -> d_shadow_hits) ->
 *     rt_path_settle_lights(that list) ->                                                                  [the last bounce ends here]
 *     rt_select_records(d_alive -> list_b+1) -> rt_cast_rays_indexed(d_next_rays, list_b+1 -> d_hits)
 * The last bounce connects and settles too, as rt_shade_hits lights the last vertex.  With the transmission queries the connection takes
 * the lobe list, as rt_path_advance does, and the settlement follows rt_path_transmit.  With the connection queries both connections of
 * a vertex are outstanding at once and need buffers of their own; the lights are settled before the sky, so that a vertex adds its
 * contributions in rt_shade_hits' order: deposit, the lights, the sky.  INTEGRATION.md writes the sequence out; DESIGN.md §3.38 has the
 * estimator, the bytes and the resources.
 *
 * The estimator.  With L_l(x) what light l sends to the vertex x through get_shade's terms, rt_shade_hits adds sum_l L_l.  This block
 * draws l with chance p_l and adds L_l / p_l: the same mean, one cast.  With a radius the light is a sphere (the area-light queries'), one
 * point of it is drawn uniformly and the light displaced there, so the mean is rt_area_light_fold's, a soft shadow.  No multiple
 * importance sampling is needed: the scene's lights are not geometry, no lobe-sampled ray ever finds one, and the connection is the only
 * strategy that reaches them.
 *
 * The streams.  With b the bounces taken, s the sample index (bounce >> 24), seed_b = seed + 0x9e3779b9u * b and seed_h =
 * film_mix(seed_b ^ 0x85ebca6bu) — rt_path_advance's — the light is chosen by u_5 = the hash of (id, film_mix(seed_h ^ 0x2545f491u), s,
 * axis 0), made as the roulette's u_3 is with a constant of its own; the point is rt_area_light_rays' d_sample for spp = 1,
 * RT_FILM_UNIFORM, that light, id, s and the seed film_mix(seed_b ^ 0x68e31da4u), bit for bit.
 *
 * Every pointer is a device pointer; both calls are stream-ordered and asynchronous on hip_stream (NULL = default stream), one kernel
 * with one listed slot per lane and 256 lanes per workgroup, allocate nothing, use no workspace, no LDS, no atomics, and may be captured
 * into a HIP graph at once.  The list is rt_path_advance's: slot j = d_index[e] for e < min(*d_count, m); an index >= m names nothing;
 * d_index NULL: every j < m, and d_count is not read.  Slots that are not listed are not touched.  d_paths is read as two 16-byte
 * accesses and never written.  All arithmetic is csrc/rt_light_connect.h's, single f32 and u32 operations in the order given here, none
 * fused, shared by both libraries.
 * Checked before any device work, in rt_path_connect's order and with its words: m >= 2^32 is RT_ERR_UNSUPPORTED; a null scene
 * (rt_path_connect_lights); m == 0 or light_count == 0 is RT_OK and launches nothing; a null pointer (d_index may be NULL; d_count only
 * with d_index; d_radii, d_weights, d_chosen and d_shadow_hits may be NULL); a d_paths that is not 16-byte aligned; then, as in
 * rt_area_light_rays, light_first + light_count beyond the scene's lights, RT_ERR_INVALID_ARGUMENT.
 * Not covered: more than one light sample per vertex; emitters that are geometry (and with them any weighing against the lobes); _host
 * and rt_multi_* forms (rt_path_connect_lights_cpu and rt_path_settle_lights_cpu of include/rt_light_connect_host.h are the CPU forms);
 * paths inside rt_render_*; any change to rt_path_advance's record or bits. */

/* The connection, per listed slot whose flags have RT_PATH_ALIVE, with d_hits[j] the path's vertex and d_incoming[j] the ray that found
 * it, before rt_path_advance moves the path.  A vertex that is "no hit" by the hit queries' rules asks nothing and draws nothing.
 * Otherwise, in this order:
 *   light      d_weights NULL: uniform, l = min((uint32_t)(u_5 * light_count), light_count - 1) and inv_p = (float)light_count.  Else
 *              d_weights holds light_count floats; one that is not > 0 counts as 0; total = their sum in ascending order in f32; l is the
 *              first light whose running sum exceeds u_5 * total (a light of weight 0 is never chosen) and inv_p = total / w_l; a total
 *              that is not > 0 asks nothing
 *   point      rt_area_light_rays' sample of light light_first + l with radius d_radii[l]; d_radii NULL or a radius that is not > 0:
 *              the stored light, no word touched
 *   ask        on the light displaced to the point, rt_light_rays' test (get_shade reaches the shadow cast) and
 *              approximate_into_directional must both hold
 *   terms      rt_light_terms' diffuse and specular of that light; e = (+0 + diffuse * (1 - shiness)) + specular * shiness, which is
 *              rt_light_fold for one light into a zeroed rgb
 *   pending    beta * (e * inv_p) per channel, each product rounded once: with one light, d_radiance + d_pending is rt_path_advance's
 *              deposit of rt_shade_hits' light, bit for bit
 *   reach      the distance from the vertex to the point, or -1.0f for a directional light without origin
 * d_asks[j] = 1 or 0; d_shadow_rays[j] = rt_light_rays' ray towards the point where it asks, all-zero words where it does not;
 * d_pending[3j ..] and d_reach[j] are written where it asks and left as they are elsewhere; d_chosen[j] (d_chosen may be NULL) = the
 * absolute index of the light drawn, whether it asks or not, or 0xffffffff where none was drawn.  Listed slots that are not alive are
 * not touched. */
int rt_path_connect_lights(const rt_scene *scene, const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count,
                           const rt_hit *d_hits, const rt_ray *d_incoming, uint32_t light_first, uint32_t light_count,
                           const float *d_radii, const float *d_weights, uint32_t seed, rt_ray *d_shadow_rays, unsigned char *d_asks,
                           float *d_pending, float *d_reach, uint32_t *d_chosen, void *hip_stream);
/* The settlement, per listed slot, alive or not (rt_path_advance may have ended the path since it connected): where d_asks[j] != 0,
 * d_radiance[3j + c] = d_radiance[3j + c] + d_pending[3j + c] unless the slot is occluded by rt_light_terms' rule — d_shadow_hits[j]'s
 * kind word is <= 1 and either d_reach[j] is negative or distance(d_shadow_rays[j].origin, d_shadow_hits[j].position) < d_reach[j]; an
 * occluder at exactly the light's distance does not occlude, and a NaN makes the compare false.  The vertex is read from the slot's own
 * shadow ray, not from d_hits.  d_shadow_hits NULL: nothing occludes.  Either way d_asks[j] = 0, so that the flags of all m slots are 0
 * again when the next bounce connects.  d_paths is not read: it is taken so that the calls share their list arguments and checks. */
int rt_path_settle_lights(const rt_path *d_paths, size_t m, const uint32_t *d_index, const uint32_t *d_count, unsigned char *d_asks,
                          const rt_ray *d_shadow_rays, const rt_hit *d_shadow_hits, const float *d_reach, const float *d_pending,
                          float *d_radiance, void *hip_stream);

/* ---- distributed (stochastic / depth-of-field) pass ----------------------------

 * Replaces the par_iter_mut closure at src/main.rs:1131-1156 and the per-pixel RNG construction at
 * main.rs:1117-1127.  rt_rng is the device-resident array of per-pixel IsaacRng states of one tile
 * (rand 0.5 IsaacRng::new_from_u64(y * 2^33 + x); 516 u32 per pixel: mem[256], a, b, c, results[256],
 * index — that is what rt_rng_download returns; on the device a pixel has two such banks, the block in use and the
 * next one, which a look-ahead pass generates before the render kernels can need it: 4128 B per pixel).  It is mutable
 * and exclusive to one render call at a time (the reference hands each pixel `&mut` access, main.rs:1131); the random
 * stream continues from call to call. */
typedef struct rt_rng rt_rng;

int rt_rng_state_words(void);
int rt_rng_create(const rt_frame *frame, rt_rng **out_rng);
int rt_rng_destroy(rt_rng *rng);
/* Copy the states to the host (rt_frame_pixels * rt_rng_state_words u32) — for tests. */
int rt_rng_download(const rt_rng *rng, uint32_t *h_states);
/* Generators that belong to no frame: n of them, generator i = IsaacRng::new_from_u64(h_seeds[i]) (host memory, uploaded once; the
 * seeding runs on the device).  rt_rng_create(frame) is the special case h_seeds[p] = y * 2^33 + x in the tile's row order
 * (main.rs:1119).  n >= 2^32 is RT_ERR_UNSUPPORTED (checked first); n == 0 gives a valid empty object, made without a device.
 * An rt_rng made either way serves wherever its count matches: a seeded one of n generators rt_trace_rays_distributed on n rays
 * and rt_focus_rays on a tile of n pixels; a frame's one the same, its generators in the tile's row order.  rt_render_distributed
 * alone wants the tile the generators were created for: a seeded rt_rng has none and is refused (RT_ERR_INVALID_ARGUMENT). */
int rt_rng_create_seeded(const uint64_t *h_seeds, size_t n, rt_rng **out_rng);
/* The inverse of rt_rng_download: rt_rng_state_words() u32 per generator in the reference's record layout (mem[256], a, b, c,
 * results[256], index), host memory.  The next render call continues exactly from those records (the device's second bank and the
 * look-ahead start afresh; so does the grouping of the pixels by cost, which only orders work).  Synchronises the device, as
 * rt_rng_download does.  Download + upload checkpoint and restore the streams. */
int rt_rng_upload(rt_rng *rng, const uint32_t *h_states);

/* n_epochs passes over the tile.  Per pixel and epoch: shoot_focus(focus, blur) (main.rs:1144-1149,
 * reference literals 3.0 / 0.04) -> cast -> distributed_ray_trace(depth = max_depth).
 *   d_accum    device, pixels*3 floats or NULL: every sample that passes the filter of main.rs:1157-1160
 *              (all three channels is_normal) is ADDED, in epoch order (img[at] = img[at] + photon,
 *              main.rs:1165).  Calling with n_epochs = 1 and running post_process in between reproduces
 *              the reference's per-epoch renormalisation (main.rs:1171).
 *   d_samples  device, n_epochs*pixels*3 floats or NULL: the raw sample of every (epoch, pixel).
 *   d_valid    device, n_epochs*pixels bytes or NULL: 1 where the sample passed the filter.
 *   d_ray_count as in rt_render_whitted.
 * At least one of d_accum / d_samples must be given. */
int rt_render_distributed(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float focus, float blur,
                          rt_rng *rng, uint32_t n_epochs, float *d_accum, float *d_samples, unsigned char *d_valid,
                          unsigned long long *d_ray_count, void *hip_stream);

/* Same, with a host image: h_accum (rt_frame_pixels * 3 floats) is uploaded, n_epochs passes are ADDED to it as above
 * and it is copied back — `img[at] = img[at] + photon` of src/main.rs:1163-1167 for n_epochs epochs in one call, which is
 * what a host that keeps `img` in its own memory binds.  *h_ray_count is overwritten with the
 * World::cast count of this call (may be NULL).  Synchronises. */
int rt_render_distributed_host(const rt_scene *scene, const rt_camera *camera, const rt_frame *frame, float focus, float blur,
                               rt_rng *rng, uint32_t n_epochs, float *h_accum, unsigned long long *h_ray_count);

/* ---- stochastic radiance queries: distributed_ray_trace on caller-supplied rays ------------------------------

 * The body of the closure at main.rs:1150-1155 with the caller's ray in place of shoot_focus's — per ray i and epoch e, in epoch
 * order, on generator i of rng:
 *     sample = match world.cast(&d_rays[i]) { Some(hit) => distributed_ray_trace(state { depth: max_depth, rng_i }, &hit), None => black }
 * (distributed_ray_trace: src/main.rs:521-614) — the stochastic scatter pass for a camera or lens model the library does not have,
 * a list of chosen pixels to resample, the secondary rays of the caller's own integrator.  Bit for bit the reference's samples,
 * flags, generator records and cast counts.
 *   d_rays       n_rays rt_ray records (device), read exactly as rt_cast_rays and rt_trace_rays read them: a face value above 2 is
 *                Both, an exclusion whose index is outside its array excludes nothing, the direction is used as given.  The ray is
 *                the same in every epoch; a fresh lens sample per epoch is rt_focus_rays + this call with n_epochs = 1.
 *   max_depth    as rt_frame.max_depth: negative renders like 0, above RT_MAX_DEPTH is RT_ERR_UNSUPPORTED.
 *   rng          n_rays generators (rt_rng_create_seeded, or a frame's of rt_frame_pixels == n_rays); generator i serves ray i and
 *                its stream continues from epoch to epoch and from call to call.
 *   d_accum      n_rays*3 floats or NULL; d_samples n_epochs*n_rays*3 floats or NULL, indexed [epoch][ray]; d_valid n_epochs*n_rays
 *                bytes or NULL; d_ray_count one u64 or NULL: all as in rt_render_distributed — the filter of main.rs:1157-1160 applies
 *                and surviving samples are ADDED to d_accum in epoch order.  Every epoch casts (and counts) its primary ray; a miss is
 *                black, which the filter rejects (0.0 is not is_normal), as in the reference.
 * Checked before any device work, in this order: n_rays >= 2^32 is RT_ERR_UNSUPPORTED; a null scene, then a null rng,
 * RT_ERR_INVALID_ARGUMENT; n_rays different from the rng's count RT_ERR_INVALID_ARGUMENT; n_rays == 0 or n_epochs == 0 is RT_OK and
 * launches nothing; a null ray pointer RT_ERR_INVALID_ARGUMENT; neither d_accum nor d_samples RT_ERR_INVALID_ARGUMENT; then max_depth.
 * The launcher is rt_render_distributed's: both organisations (rt_set_distributed_split) with the same bits, batches of epochs, the
 * two workspaces, the look-ahead, rt_profile_read_distributed and every RT_AMD_DIST_* switch; a batch of more than 2^26 rays runs
 * in bands of whole 64-ray chunks.  Stream-ordered and asynchronous on hip_stream as rt_render_distributed is.  Graph capture is
 * supported by neither of the two: a call forks onto streams the rt_rng owns, keeps host-side look-ahead state per call and may
 * allocate its workspace.  A wave takes 64 consecutive rays: rays that travel together should be neighbours. */
int rt_trace_rays_distributed(const rt_scene *scene, const rt_ray *d_rays, size_t n_rays, int32_t max_depth, rt_rng *rng, uint32_t n_epochs,
                              float *d_accum, float *d_samples, unsigned char *d_valid, unsigned long long *d_ray_count, void *hip_stream);
/* Same, with host rays and a host image: h_accum (n_rays*3 floats, required) is uploaded, added to as above and copied back;
 * *h_ray_count is overwritten with the cast count of this call (may be NULL).  Synchronises.  Without a device it fails with a
 * status and writes nothing. */
int rt_trace_rays_distributed_host(const rt_scene *scene, const rt_ray *h_rays, size_t n_rays, int32_t max_depth, rt_rng *rng,
                                   uint32_t n_epochs, float *h_accum, unsigned long long *h_ray_count);
/* The library's lens as a ray source: for every pixel of the tile, in compact row order as rt_camera_rays, d_rays[p] =
 * Camera::shoot_focus(clip(x, y), state, focus, blur) (main.rs:101-127), the two Normal(0, blur) values drawn from that pixel's
 * generator, which advances.  rng: the frame's, or a seeded one of rt_frame_pixels generators.  Face Front, no exclusion; the ray is
 * bit for bit the one rt_render_distributed casts first, so one rt_focus_rays + rt_trace_rays_distributed(n_epochs = 1) IS one epoch
 * of rt_render_distributed — and the caller may transform, reorder, subset or replace the rays in between.  frame->max_depth is
 * not used.  Stream-ordered on hip_stream. */
int rt_focus_rays(const rt_camera *camera, const rt_frame *frame, float focus, float blur, rt_rng *rng, rt_ray *d_rays, void *hip_stream);

/* ---- scatter queries: weighted_select and scatter_hit on caller-supplied hits ------------------------------

 * The three generator draws distributed_ray_trace (main.rs:521-614) makes per level before it calls get_reflect or get_refract, and
 * the level's factor once the next ray is known — with the hit queries above, everything a caller needs to run the depth-of-field and
 * scatter integrator one level at a time: cast -> scatter -> reflect / refract -> cast -> shade and factor, with its own stopping
 * rule, weighting, re-sorting or mix of levels (INTEGRATION.md writes the loop and the fold out).  Every bit, every generator record
 * and every cast is the reference's.  Records are the hit queries': entry i of d_incoming is Hit.ray of entry i of d_hits; device
 * pointers; stream-ordered and asynchronous on hip_stream.  The record rules are those of the hit-query block:
 *   - a hit whose kind is neither 0 nor 1, or whose object_index >= n_materials, is "no hit"; so is (rt_scatter_hits) a record whose
 *     generator index is at or beyond the rt_rng's count.  A "no hit" record writes type RT_HIT_NONE, an all-zero ray, cosine 0 and a
 *     black factor — and DRAWS NOTHING: its generator does not move.  That is how a caller masks dead or finished records without
 *     compacting;
 *   - a valid record always draws exactly three u32 words, as the reference does, in the order selection, phi, theta.  The depth test
 *     of main.rs:525 stays with the caller: it makes no draw;
 *   - incoming rays are read as rt_cast_rays reads them; NaN and Inf pass through the arithmetic; degenerate materials (a NaN weight,
 *     a weight sum that is not positive, where the reference would panic) give what rt_trace_rays_distributed gives: it is the same code;
 *   - d_rng_index == NULL means record i draws from generator i; then n must equal the generator count (RT_ERR_INVALID_ARGUMENT).  With
 *     an index array n is free: a caller may compact or re-sort its records between levels and keep each on its own stream.  Two
 *     records of one call naming the same generator is the caller's error: their results are unspecified, the call stays memory-safe.
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene, then (rt_scatter_hits) a null rng,
 * RT_ERR_INVALID_ARGUMENT; the count mismatch above; n == 0 is RT_OK and launches nothing; a null record pointer or a null required
 * output pointer RT_ERR_INVALID_ARGUMENT.  A batch of more than 2^26 records runs in bands of whole 64-record chunks
 * (RT_AMD_DIAG_HIT_BAND_RECORDS shortens them for tests).  rt_scatter_factors uses no workspace and no generator and may be captured
 * into a HIP graph at once.  rt_scatter_hits mutates an rt_rng: calls on one rt_rng must be serialised by the caller, and a later
 * rt_trace_rays_distributed, rt_render_distributed, rt_focus_rays or rt_rng_download continues bit-exactly from where it left the
 * streams.  A generator that runs dry (every 256 words: about every 85 calls) generates its next block inside the kernel;
 * RT_AMD_SCATTER_PREPARE=1 runs the look-ahead pass ahead of the kernel instead (same bits; DESIGN.md §3.11 has the measurement).
 * Not covered: rt_multi_* variants; per-record cast counts (these two calls cast nothing).  The device-side fold is
 * rt_level_fold, in the level-loop block below. */

#define RT_SCATTER_DIFFUSE 0u
#define RT_SCATTER_REFLECTION 1u
#define RT_SCATTER_REFRACTION 2u
/* per record i, on generator g = d_rng_index ? d_rng_index[i] : i of rng, in stream order:
 *   type   = weighted_select(rng_g, [(1-shiness)(1-transparency), shiness(1-transparency), transparency])   main.rs:533-537, 652-666
 *   s_hit  = scatter_hit(state, hit, type == Diffuse ? -hit.normal : hit.ray.direction,
 *                        type == Diffuse ? 1.0 : material.smoothness)                                       main.rs:539-554
 *   d_type[i]      0 Diffuse, 1 Reflection, 2 Refraction; RT_HIT_NONE for a record that is "no hit"
 *   d_scattered[i] s_hit.ray: the incoming rt_ray with its direction replaced by new_dir (origin, face mode and exclusion copied, as
 *                  hit.clone() does; a face value above 2 is written as 2, as it was read), so (d_hits[i], d_scattered[i]) IS
 *                  scattered_hit and feeds rt_reflect_rays / rt_refract_rays / rt_shade_hits as it is
 *   d_cosine[i]    -hit.normal . new_dir (main.rs:559, 578, 597); the caller tests `cosine <= 0` (may be NULL) */
int rt_scatter_hits(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, size_t n, rt_rng *rng,
                    const uint32_t *d_rng_index, uint32_t *d_type, rt_ray *d_scattered, float *d_cosine, void *hip_stream);
/* the level's factor once the next ray is known (main.rs:566-570, 585-589, 605), d_rgb[3*i + c]:
 *   type 0: material.get_diffuse (probe { at: hit.at, view: -d_incoming[i].direction, light: d_next[i].direction })
 *   type 1: material.get_specular(the same probe)
 *   type 2: opaque_decay.powf(d_travel[i]) in all three channels
 *   any other type, or a record that is "no hit": 0
 * d_next: the ray the level cast next (rt_reflect_rays' output, or the escape ray); d_travel: rt_refract_rays' d_travel.  All six
 * pointers are required; d_next[i] is read for types 0 and 1 only and d_travel[i] for type 2 only. */
int rt_scatter_factors(const rt_scene *scene, const rt_hit *d_hits, const rt_ray *d_incoming, const uint32_t *d_type,
                       const rt_ray *d_next, const float *d_travel, size_t n, float *d_rgb, void *hip_stream);
/* The same two with host records in and out: allocate, launch, copy back and synchronise.  The rng stays a device object, as in
 * rt_trace_rays_distributed_host; h_rng_index and h_cosine may be NULL as above.  Without a device they fail with a status and write
 * nothing. */
int rt_scatter_hits_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, size_t n, rt_rng *rng,
                         const uint32_t *h_rng_index, uint32_t *h_type, rt_ray *h_scattered, float *h_cosine);
int rt_scatter_factors_host(const rt_scene *scene, const rt_hit *h_hits, const rt_ray *h_incoming, const uint32_t *h_type,
                            const rt_ray *h_next, const float *h_travel, size_t n, float *h_rgb);

/* ---- level loop: select, indexed casts, the glue of one level and the fold, on the device ------------------------------

 * What lies BETWEEN two queries when a caller runs distributed_ray_trace (main.rs:521-614) one level at a time: which records still have
 * a ray, a cast of those alone, the masks of main.rs:556-613 as records the hit queries take, and the unwind — so that one epoch of the
 * loop is a fixed sequence of stream-ordered calls: the host reads nothing back and does no arithmetic between the primary cast and the
 * finished sample, and the result is rt_trace_rays_distributed's bit for bit (INTEGRATION.md writes the sequence out).  The primitives
 * are generic: a caller's own stopping or re-sorting rule uses the same selection and the same indexed cast.
 * Every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream).  Records are
 * the caller's and are validated, never trusted: a type above 2 belongs to no branch (RT_HIT_NONE is the dead record); a next hit whose
 * kind is neither 0 nor 1 is a miss; an index at or beyond n is skipped.
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED (for rt_cast_rays_indexed max_count >= 2^32 as well);
 * a null scene RT_ERR_INVALID_ARGUMENT (rt_cast_rays_indexed); n == 0 is RT_OK and launches nothing (so rt_select_records leaves *d_count
 * as it was; for rt_cast_rays_indexed max_count == 0 as well); a null required pointer RT_ERR_INVALID_ARGUMENT.
 * Any n below 2^32 runs in one launch per kernel (the record number is counted in 64 bits; no bands).
 * Not covered: rt_multi_* forms; indexed forms of the hit and scatter queries, which already skip "no hit" records; per-record cast
 * counts.  The Whitted recursion, a tree and not a chain, has its own glue and fold in the tree-loop block below. */

/* Stable selection: d_index[0 .. *d_count) receives, ascending, every i with d_flags[i] != 0 (any non-zero byte); *d_count (one u32) is
 * overwritten with their number and never goes to the host.  d_index has room for n words; entries at and beyond the count are
 * unspecified.  Records that were neighbours stay neighbours: what keeps the 64 rays of a wave together.  The same flags always give
 * the same output: two kernels (block totals, then the placement: a workgroup's base is the sum of the totals before it), no ordering by
 * atomics.  The totals live in a 4 KB scratch per (device, stream), allocated by the first call on that stream — which therefore must not
 * be captured (RT_ERR_UNSUPPORTED if it is); every later call on the stream may be captured into a HIP graph.  rt_post_release frees
 * the scratch of the current device. */
int rt_select_records(const unsigned char *d_flags, size_t n, uint32_t *d_index, uint32_t *d_count, void *hip_stream);

/* World::cast through an index list: for j < min(*d_count, max_count), with k = d_index[j]: d_hits[k] = World::cast(d_rays[k]), bit for
 * bit what rt_cast_rays writes for that ray, NaN distances included.  Records that are not named are not written; an index >= n is
 * skipped (nothing is read or cast for it).  d_rays and d_hits hold n records; max_count is the host's upper bound on the list's length
 * (typically n): it sizes the grid, and waves beyond the device-side count leave at once.  A wave takes 64 consecutive index entries.
 * An index named twice is cast twice and written twice, with the same bits.  d_ray_count: NULL or one u64, the number of casts actually
 * made is ADDED.  Routes and graph capture as rt_cast_rays: pair-wise, or wave-uniform under RT_AMD_QUERY_WAVE_UNIFORM=1, no workspace;
 * a scene walked breadth-first takes the breadth-first walk with the record lists of the per-(scene, stream) workspace (make one
 * uncaptured call on the stream first, with at least as large a max_count; a call captured before that uses the pair-wise kernel). */
int rt_cast_rays_indexed(const rt_scene *scene, const rt_ray *d_rays, size_t n, const uint32_t *d_index, const uint32_t *d_count,
                         size_t max_count, rt_hit *d_hits, unsigned long long *d_ray_count, void *hip_stream);

/* The glue of one level.  With type and cosine as rt_scatter_hits wrote them:
 *     alive(i) = d_type[i] != RT_HIT_NONE && !(d_cosine[i] <= 0)      (a NaN cosine goes on, as in the reference: main.rs:559, 578, 597)
 *     dr(i) = alive && d_type[i] <= 1 (Diffuse, Reflection)           fr(i) = alive && d_type[i] == 2 (Refraction)
 * "no hit" is kind RT_HIT_NONE with every other word 0, as rt_cast_rays writes a miss.  Each call is one element-wise kernel, needs no
 * workspace and may be captured at once.  All pointers are required unless said otherwise; n records each.
 *   rt_level_split   after rt_scatter_hits: d_hits_reflect[i] = d_hits[i] where dr, d_hits_refract[i] = d_hits[i] where fr, "no hit"
 *                    elsewhere — the operands of rt_reflect_rays and rt_refract_rays (with d_scattered as their incoming rays)
 *   rt_level_join    after those two: d_next[i] = d_reflected[i] where dr, d_escape[i] where fr && d_refr_kind[i] == 0 (Escaped), all-zero
 *                    words elsewhere; d_flags[i] = 1 exactly where such a ray exists, else 0; d_next_hits[i] is preset to "no hit" for
 *                    every i — rt_select_records(d_flags) + rt_cast_rays_indexed(d_next -> d_next_hits) then overwrite the records cast
 *   rt_level_close   after the indexed cast: d_hits_missed[i] = d_hits[i] where dr and d_next_hits[i].kind is neither 0 nor 1, "no hit"
 *                    elsewhere — the operand of get_shade(&scattered_hit) (main.rs:573, 592; incoming rays: d_scattered)
 *   rt_level_fold    from the deepest level back, d_value (3 floats per record) holding the value of the level below (at the deepest:
 *                    rt_shade_hits of the last hits) and receiving this level's, in place:
 *                        !alive, or a type above 2                black                                       (main.rs:560, 579, 598)
 *                        type <= 1, next kind 0 or 1              s = value * factor; shade_next + (s - shade_next) * 0.5 per channel
 *                        type <= 1, otherwise                     shade_missed                                (main.rs:573, 592)
 *                        type == 2, next kind 0 or 1              (value + shade_next) * factor[0] in all three channels (main.rs:605)
 *                        type == 2, otherwise                     black                                       (main.rs:607-611)
 *                    d_factor: rt_scatter_factors; d_shade_next: rt_shade_hits(d_next_hits, d_next); d_shade_missed:
 *                    rt_shade_hits(d_hits_missed, d_scattered).  Every operation rounds to f32, none is fused: the operations and
 *                    their order are those of rt_trace_rays_distributed's unwind
 *   rt_level_finish  main.rs:1157-1165: valid = all three channels of d_value[i] are is_normal; d_valid[i] = valid (one byte; may be NULL);
 *                    d_accum[3*i + c] += d_value[3*i + c] where valid (may be NULL).  Neither: RT_ERR_INVALID_ARGUMENT */
int rt_level_split(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, size_t n, rt_hit *d_hits_reflect, rt_hit *d_hits_refract,
                   void *hip_stream);
int rt_level_join(const uint32_t *d_type, const float *d_cosine, const rt_ray *d_reflected, const uint32_t *d_refr_kind, const rt_ray *d_escape,
                  size_t n, rt_ray *d_next, rt_hit *d_next_hits, unsigned char *d_flags, void *hip_stream);
int rt_level_close(const rt_hit *d_hits, const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, size_t n, rt_hit *d_hits_missed,
                   void *hip_stream);
int rt_level_fold(const uint32_t *d_type, const float *d_cosine, const rt_hit *d_next_hits, const float *d_factor, const float *d_shade_next,
                  const float *d_shade_missed, size_t n, float *d_value, void *hip_stream);
int rt_level_finish(const float *d_value, size_t n, float *d_accum, unsigned char *d_valid, void *hip_stream);

/* ---- tree loop: ray_trace level by level on the device — gate, split, spawn, gather and fold ------------------------------

 * What lies BETWEEN two queries when a caller runs the Whitted integrator ray_trace (main.rs:466-519) one level at a time.  The
 * stochastic loop above is a chain: one successor per record.  ray_trace is a tree with up to two children per node (the reflected
 * ray and the escape ray of the refraction), so it needs three things the chain never did: the material weights and threshold gates
 * of main.rs:480-504 as a query, the compaction of 2n child candidates into the next level with a link to the parent's slot, and a
 * fold that hands each child's value to that slot.  rt_select_records and rt_cast_rays_indexed are used as they are.  One level is
 *     [roots] rt_tree_gate -> rt_select_records -> rt_cast_rays_indexed        [children] rt_cast_rays_indexed (identity list, level count)
 *     rt_tree_split -> rt_shade_hits, rt_reflect_rays, rt_refract_rays(100.0)   (incoming rays: the level's rays)
 *     rt_tree_spawn -> rt_select_records(2n flags) -> rt_tree_gather            (not at depth_left <= 0)
 * and, from the deepest level back, rt_tree_fold.  The host reads nothing back and does no arithmetic, and values and cast count are
 * rt_trace_rays' bit for bit (INTEGRATION.md writes the sequence out; DESIGN.md §3.13 says why the bits are the same).
 * Rules of the block: every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default
 * stream), is one element-wise kernel with one record per lane, uses no workspace and may be captured into a HIP graph at once.  n is
 * the CAPACITY of the level's arrays; d_count is one device u32 holding the number of live records (a count above n is read as n), it
 * never goes to the host, and a NULL d_count means n.  Records at or beyond the count are dead: they are read as "no hit" and written
 * as "no hit", zero or not at all, as said per call.  Records are the caller's and are validated, never trusted: a hit whose kind is
 * neither 0 nor 1 is "no hit", and so is (rt_tree_split) one whose object_index >= n_materials.  "no hit" is kind RT_HIT_NONE with
 * every other word 0.  Checked before any device work, in this order: the limit on n (per call, below) is RT_ERR_UNSUPPORTED; a null
 * scene RT_ERR_INVALID_ARGUMENT (rt_tree_split); n == 0 is RT_OK and launches nothing; a null required pointer RT_ERR_INVALID_ARGUMENT.
 * Not covered: rt_multi_* forms; per-record cast counts. */

/* The entry check of main.rs:469 on the roots: d_flags[j] = j < count && !(d_contribution[j] < 0.001f) — a NaN contribution passes, as
 * in the reference — and d_hits[j] is preset to "no hit" for every j < n; rt_select_records(d_flags) + rt_cast_rays_indexed then cast the
 * roots that passed.  Child levels need no gate: a child exists only where contribution * weight passed the threshold.
 * n >= 2^32 is RT_ERR_UNSUPPORTED. */
int rt_tree_gate(const float *d_contribution, size_t n, const uint32_t *d_count, unsigned char *d_flags, rt_hit *d_hits, void *hip_stream);

/* main.rs:478-504 up to the three calls.  With the hit's material (material.approx(hit.at)), in f32 and in the reference's order:
 *     sc = (1 - shiness) * (1 - transparency)     rc = shiness * (1 - transparency)     fc = transparency
 * and c = d_contribution[j], a live record (j < count and a valid hit) copies its hit to
 *     d_hits_shade[j]    where c * sc >= 0.001f                           the operand of rt_shade_hits
 *     d_hits_reflect[j]  where depth_left > 0 && c * rc >= 0.001f         the operand of rt_reflect_rays
 *     d_hits_refract[j]  where depth_left > 0 && c * fc >  0.001f         the operand of rt_refract_rays (strict, main.rs:504)
 * and everywhere else, for every j < n, the three outputs are "no hit".  d_weights[4*j ..] = (sc, rc, fc, opaque_decay), zeros for a
 * record that is not live.  depth_left: TraceState.depth of the level, uniform.  n >= 2^32 is RT_ERR_UNSUPPORTED. */
int rt_tree_split(const rt_scene *scene, const rt_hit *d_hits, const float *d_contribution, size_t n, const uint32_t *d_count, int32_t depth_left,
                  rt_hit *d_hits_shade, rt_hit *d_hits_reflect, rt_hit *d_hits_refract, float *d_weights, void *hip_stream);

/* The child candidates of a level, two per record: d_flags[2*j] = d_hits_reflect[j] is a hit (the reflection child), d_flags[2*j + 1] =
 * d_refr_kind[j] == 0 (Escaped: the refraction child); d_child_values (6 floats per record: 3 per candidate) is zeroed — black until the
 * child's fold overwrites its slot.  rt_select_records(d_flags, 2n) then lists the candidates ascending: siblings stay adjacent and
 * children stay in their parents' order, which keeps a wave's rays together.  n >= 2^31 is RT_ERR_UNSUPPORTED (2n stays below 2^32). */
int rt_tree_spawn(const rt_hit *d_hits_reflect, const uint32_t *d_refr_kind, size_t n, unsigned char *d_flags, float *d_child_values,
                  void *hip_stream);

/* The next level from the selected candidates.  For j < min(*d_count, max_count), with c = d_index[j], p = c >> 1, slot = c & 1:
 *     d_child_rays[j] = slot ? d_escape[p] : d_reflected[p]
 *     d_child_contribution[j] = d_contribution[p] * (slot ? fc : rc) of d_weights[4*p ..]    (one f32 multiply: TraceState::nested)
 *     d_child_parent[j] = c
 * *d_child_count = min(*d_count, max_count), and the number of candidates that did not fit is ADDED to *d_overflow (one u32): their
 * parents see a black child and the call stays memory-safe.  max_count is the capacity of the child arrays; n the parents' capacity
 * (d_index comes from rt_select_records over 2n flags: it holds at least min(max_count, 2n) entries).  An index c >= 2n names no candidate: its record is an all-zero ray with
 * contribution 0 and parent 0xffffffff, which folds into no slot.  d_child_count must not alias d_count.  Checked first:
 * n >= 2^31 or max_count >= 2^32 is RT_ERR_UNSUPPORTED.  With max_count == 0 the child arrays may be NULL. */
int rt_tree_gather(const uint32_t *d_index, const uint32_t *d_count, size_t max_count, const rt_ray *d_reflected, const rt_ray *d_escape,
                   const float *d_contribution, const float *d_weights, size_t n, rt_ray *d_child_rays, float *d_child_contribution,
                   uint32_t *d_child_parent, uint32_t *d_child_count, uint32_t *d_overflow, void *hip_stream);

/* main.rs:516-518 on one level, from the deepest back.  For every j < count the value is
 *     not live (a miss, a gated root)     +0 black                                                       (main.rs:470, 475)
 *     depth_left <= 0                     d_shade[3*j ..] as rt_shade_hits wrote it, NOT multiplied by sc  (main.rs:488-490)
 *     otherwise                           (shade * sc + reflection * rc) + refraction * fc               (main.rs:516-518)
 * with reflection = d_child_values[6*j ..], refraction = d_child_values[6*j + 3 ..] * powf(opaque_decay, d_travel[j]) where
 * d_refr_kind[j] == 0 and black, without the multiply, elsewhere (main.rs:508-510); the powf is the library's deterministic one
 * (rt_math_eval_host(RT_MATH_POW)).  Every operation rounds to f32, none is fused, and the association is rt_trace_rays'.  A shade that
 * was not wanted is black and is still multiplied by sc.  Live is j < count and d_hits[j].kind <= 1 (a hit rt_tree_split rejected for its
 * object_index has black shade and zero weights: +0 either way).  The value goes to d_out[3*d_parent[j] + c] — d_out being the parent
 * level's d_child_values, 3 floats per candidate — or, with d_parent == NULL (the roots), to d_out[3*j + c].  n_out is the number of
 * 3-float slots d_out holds: a parent at or beyond it writes nothing.  Each slot has one writer: no atomics, and the result does not
 * depend on scheduling.  Dead records write nothing.  d_weights, d_refr_kind, d_travel and d_child_values may be NULL when
 * depth_left <= 0.  n >= 2^32 is RT_ERR_UNSUPPORTED. */
int rt_tree_fold(const rt_hit *d_hits, const uint32_t *d_count, size_t n, int32_t depth_left, const float *d_shade, const float *d_weights,
                 const uint32_t *d_refr_kind, const float *d_travel, const float *d_child_values, const uint32_t *d_parent, float *d_out,
                 size_t n_out, void *hip_stream);

/* ---- record ordering: coherence keys, a stable sort of an index list, gather and scatter ------------------------------
 * Every query block above says that a wave takes 64 consecutive records and that rays which travel together should be neighbours, and
 * leaves the order to the caller.  This block builds such an order on the device: a coherence key per ray, a stable and deterministic
 * radix sort of an index list by caller keys — the list rt_cast_rays_indexed takes — and a gather and a scatter of fixed-size records
 * through a list, for the calls that take none (rt_trace_rays, the hit and scatter queries).  INTEGRATION.md writes the two sequences
 * out; DESIGN.md §3.17 describes the kernels.
 * Rules of the block: every data pointer is a device pointer unless said otherwise; every call is stream-ordered and asynchronous on
 * hip_stream (NULL = default stream), allocates nothing and may be captured into a HIP graph at once; records and lists are the
 * caller's and are validated, never trusted: a list entry at or beyond n names no record.  A device-side count never goes to the host:
 * grids are sized from the host's bound, and waves beyond the count leave at once.
 * Checked before any device work, in this order: n >= 2^32 (and max_count >= 2^32) is RT_ERR_UNSUPPORTED; n == 0 (or max_count == 0)
 * is RT_OK and launches nothing; a null required pointer is RT_ERR_INVALID_ARGUMENT; then the values, each RT_ERR_INVALID_ARGUMENT: the
 * flags, key_bits == 0 or first_bit + key_bits > 32, record_bytes, temp_bytes, a d_count_in given without d_index_in.
 * Not covered: rt_multi_* forms; 64-bit keys; sorting inside the render kernels; indexed forms of the hit and scatter queries, since
 * gather and scatter serve them. */

#define RT_ORDER_DIRECTION_MAJOR 1u /* rt_ray_keys: the direction code above the origin code */

/* A 30-bit coherence key per ray; no scene is read.  box_lo and box_hi are HOST arrays of 3 floats (the scene's bounds, or any box the
 * caller likes); per axis scale[a] = hi > lo ? 64.0f / (hi - lo) : 0.0f, a NaN giving 0.  Per ray, every operation a single f32 operation
 * in the order written, nothing fused:
 *     cell(t)  = 0 if t is NaN or t < 0;  63 if t >= 63;  (uint32)t, truncated, otherwise
 *     origin   x, y, z = cell((o[a] - lo[a]) * scale[a])
 *     direction, used as given: s = (|dx| + |dy|) + |dz|, px = dx / s, py = dy / s; if dz < 0.0f (strict: -0.0 and NaN do not fold)
 *              the pair becomes ((1 - |py|) * sg(px), (1 - |px|) * sg(py)), both from the old values, sg(x) = x >= 0.0f ? 1.0f : -1.0f;
 *              u = cell((px * 0.5f + 0.5f) * 64.0f), v likewise from py                       (the octahedral map, 64 x 64 cells)
 *     ocode    bit k of x, y, z at bit 3k, 3k + 1, 3k + 2 (18 bits);  dcode  bit k of u, v at bit 2k, 2k + 1 (12 bits)
 *     key      (ocode << 12) | dcode, or with RT_ORDER_DIRECTION_MAJOR (dcode << 18) | ocode; bits 30 and 31 are zero
 * Any other flag bit is RT_ERR_INVALID_ARGUMENT.  Face and exclusion words are not read.  Rays of one origin sort by dcode, a Z-order
 * over the octahedral map: camera rays come out in tile-like order; rays leaving surfaces sort by where they start. */
int rt_ray_keys(const rt_ray *d_rays, size_t n, const float box_lo[3], const float box_hi[3], uint32_t flags, uint32_t *d_keys, void *hip_stream);

/* Stable LSD radix sort of an index list by bits [first_bit, first_bit + key_bits) of d_keys[index], ascending; equal keys keep their
 * input order.  d_keys is any array of n u32: rt_ray_keys' output, or the caller's own (rt_scatter_hits' d_type with key_bits = 2 groups
 * a level by branch; first_bit = 12, key_bits = 18 orders rt_ray_keys' default key by origin cell alone).
 * The input list: d_index_in == NULL is the identity list 0 .. n-1 (d_count_in must be NULL too); otherwise d_index_in[0 .. m) with
 * m = min(*d_count_in, n), a NULL d_count_in meaning n.  d_index_out[0 .. m) receives the permuted list; entries at and beyond m are
 * unspecified and no more than n words are ever written.  An entry >= n reads no key, sorts behind every valid entry and keeps its
 * value (rt_cast_rays_indexed and rt_gather_records skip it); entries naming the same record are kept, adjacent, in input order.
 * d_index_out may alias d_index_in.  The same inputs always give the same output: placement is by ranks — per-tile digit counts, a scan,
 * in-tile ranks from ballots and LDS; atomics count but never order.  ceil(key_bits / 8) passes of three kernels each.
 * d_temp: rt_sort_temp_bytes(n) bytes of the caller's, 4-byte aligned, contents unspecified before and after; a smaller temp_bytes is
 * RT_ERR_INVALID_ARGUMENT.  rt_sort_temp_bytes is host arithmetic, monotone in n, and 0 for n == 0 and for n >= 2^32. */
size_t rt_sort_temp_bytes(size_t n);
int rt_sort_records(const uint32_t *d_keys, size_t n, uint32_t first_bit, uint32_t key_bits, const uint32_t *d_index_in, const uint32_t *d_count_in,
                    uint32_t *d_index_out, void *d_temp, size_t temp_bytes, void *hip_stream);

/* Fixed-size records through a list, as dwords: record_bytes is a multiple of 4 in 4..256 (rt_ray 44, rt_hit 52, rgb 12, a flag word 4)
 * and the arrays are 4-byte aligned.  Both calls cover j < min(*d_count, max_count), a NULL d_count meaning max_count.
 *   rt_gather_records    d_dst[j] = d_src[d_index[j]], all-zero words where d_index[j] >= n; d_src holds n records, d_dst max_count
 *   rt_scatter_records   d_dst[d_index[j]] = d_src[j], an index >= n is skipped; d_src holds max_count records, d_dst n.  Of two entries
 *                        with the same index either source may win, word by word; the call stays memory-safe
 * d_src and d_dst must not overlap. */
int rt_gather_records(const void *d_src, size_t record_bytes, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count,
                      void *d_dst, void *hip_stream);
int rt_scatter_records(const void *d_src, size_t record_bytes, size_t n, const uint32_t *d_index, const uint32_t *d_count, size_t max_count,
                       void *d_dst, void *hip_stream);

/* ---- mesh ordering: triangle keys and the permutation that makes the node tree selective ------------------------------
 * rt_scene_create builds its node tree over the triangles IN THE ORDER GIVEN: within each run of equal object_index a leaf is 16
 * consecutive triangles, leaves are grouped 16 by 16, and a node can be skipped only if its bounding sphere is small and its plane
 * directions are few or lie in a narrow cone.  A mesh whose consecutive triangles are neighbours on the surface (a subdivision that
 * emits siblings together) gets such nodes; an exporter's face order, a simulation's particle order or a concatenation of parts
 * does not — every leaf spans the object, nothing is skipped, and the walk is brute force.  This block produces the order: a Z-order
 * key per triangle and, from the record ordering above, the stable permutation by (object_index, key).
 * The order is a tool the caller applies, never rt_scene_create behind the caller's back: every entry point reports primitive
 * indices, and among accepted triangles at equal distance World::cast keeps the later one (main.rs:229-233), so a reordered
 * description is ANOTHER SCENE.  Each of the two is bit-identical to the reference's cast of its own description; mapped through the
 * permutation they agree everywhere except at such ties (same distance bits, another triangle).  The permutation is handed back so
 * that indices can be mapped: hits back through d_perm, a ray's triangle exclusion forward through its inverse.
 * The same call serves a scene that rt_scene_update_vertices has deformed until its nodes no longer reject: order the moved
 * description and re-create.  Re-clustering a live scene in place is not covered.
 * Rules as in the record-ordering block: device pointers unless said otherwise, stream-ordered on hip_stream, no allocation, may be
 * captured into a HIP graph at once.  Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; n == 0 is RT_OK
 * and launches nothing; a null required pointer is RT_ERR_INVALID_ARGUMENT; then temp_bytes, RT_ERR_INVALID_ARGUMENT.
 * Not covered: ordering inside rt_scene_create, or original indices kept inside the kernels; spheres; rt_multi_* forms; 64-bit keys. */

/* A 30-bit key per triangle: the cell of its centroid in a 1024^3 grid over the box, in Z-order.  box_lo and box_hi are HOST arrays of
 * 3 floats (World.bounds, or any box); per axis scale[a] = hi > lo ? 1024.0f / (hi - lo) : 0.0f, a NaN giving 0.  Per triangle with
 * vertex positions p0, p1, p2, every operation a single f32 operation in the order written, nothing fused:
 *     c[a]     = ((p0[a] + p1[a]) + p2[a]) / 3.0f
 *     cell(t)  = 0 if t is NaN or t < 0;  1023 if t >= 1023;  (uint32)t, truncated, otherwise
 *     x, y, z  = cell((c[a] - lo[a]) * scale[a])
 *     key      = bit k of x, y, z at bit 3k, 3k + 1, 3k + 2; bits 30 and 31 are zero
 * NaN, infinite and degenerate triangles get a cell by these rules.  d_objects, which may be NULL, receives d_triangles[i].object_index.
 * Only the positions and the object word are read (as dwords: an rt_triangle is 100 bytes and 4-byte aligned). */
int rt_triangle_keys(const rt_triangle *d_triangles, size_t n, const float box_lo[3], const float box_hi[3], uint32_t *d_keys, uint32_t *d_objects,
                     void *hip_stream);

/* The whole sequence as one call: rt_triangle_keys; rt_sort_records of the identity list by the 30 key bits; a second, stable
 * rt_sort_records of that list by object_index over max(1, bits of n_objects - 1) bits; and, with d_ordered_or_null given,
 * rt_gather_records(d_triangles, 100, ...) into it.  d_perm[j] (n words) is the OLD index of the triangle at NEW position j: the list
 * is grouped by object, ascending, and inside an object it is in Z-order of the centroid cells; equal (object, key) pairs keep their
 * input order.  The same inputs always give the same words.  d_ordered_or_null (n records) must not overlap d_triangles.
 * n_objects is the description's n_materials.  An object_index >= n_objects cannot be refused here, since the records are on the
 * device: such triangles sort by the low bits of their object word, and rt_scene_create rejects the description as it always did.
 * d_temp: rt_order_triangles_temp_bytes(n) bytes, 4-byte aligned — the keys, the object words and rt_sort_temp_bytes(n) — contents
 * unspecified before and after; the size is host arithmetic, monotone in n, and 0 for n == 0 and for n >= 2^32. */
size_t rt_order_triangles_temp_bytes(size_t n);
int rt_order_triangles(const rt_triangle *d_triangles, size_t n, const float box_lo[3], const float box_hi[3], uint32_t n_objects, uint32_t *d_perm,
                       rt_triangle *d_ordered_or_null, void *d_temp, size_t temp_bytes, void *hip_stream);
/* The same on HOST arrays: allocates, copies, runs, synchronises the device and copies back (h_perm: n words; h_ordered_or_null: n
 * records or NULL).  Without a device it returns the status and writes nothing. */
int rt_order_triangles_host(const rt_triangle *h_triangles, size_t n, const float lo[3], const float hi[3], uint32_t n_objects, uint32_t *h_perm,
                            rt_triangle *h_ordered_or_null);

/* ---- scene updates: move triangles, spheres and lights in place ------------------------------
 * An animated sequence changes the world between two frames without rt_scene_destroy + rt_scene_create: the device arrays are
 * rewritten in place, so the scene's pointers, its per-stream workspaces and every captured graph that names it stay valid.  After
 * an update every render and query entry point gives, bit for bit, what it gives on a scene freshly created from the updated
 * description: the values the reference computes per primitive (face normal, plane constant, edges, area, squared radius) are
 * recomputed on the device in the reference's operation order, and everything the intersection loop only uses to leave work out
 * (bounding spheres, the node tree's spheres, normals and cones, the plane-sharing bits) is refitted by the rules
 * rt_scene_create builds it by.
 *
 * What never changes: the NUMBER of triangles, spheres, lights and materials, every object_index, and the node tree's topology (which
 * triangles share a node) — a caller who needs one of them changed re-creates the scene.  The scene's box is the one it was created
 * with: geometry that moves outside it (a coordinate larger in magnitude than the largest at creation) is rendered correctly but
 * loses its rejections, and so does every node above it — correct, slower; moving back restores them.  A node whose triangles no
 * longer qualify (a sliver, a degenerate or non-finite triangle, a normal cone of 60 degrees or more) is always visited until they
 * do again.  The tree is not re-clustered: after a deformation that scatters the triangles of a node, a fresh rt_scene_create
 * of the description put in order again (rt_order_triangles, "mesh ordering" above) may render faster.  Not covered: the rt_multi_* forms (their scenes are re-created).
 *
 * All four calls are stream-ordered on hip_stream.  The scene's arrays are shared by ALL streams: ordering a render or a query on
 * another stream after an update (or an update after a render still in flight elsewhere) is the caller's business — an event —
 * as with any buffer.
 * Checks, in this order and before any device work: a null scene is RT_ERR_INVALID_ARGUMENT; first + count (in 64 bits) beyond the
 * array is RT_ERR_INVALID_ARGUMENT; count == 0 is RT_OK and launches nothing; a null data pointer is RT_ERR_INVALID_ARGUMENT.
 *
 * rt_scene_update_vertices: d_vertices holds 3 * count rt_vertex records in DEVICE memory, the three vertices of triangles
 * first .. first + count - 1 (positions, normals and uvs all replace the old ones).  The per-triangle records of the range are
 * rewritten and the node tree of the WHOLE scene is refitted (whether a node qualifies depends on every triangle below it).  The
 * first call on a scene allocates (the nodes' triangle ranges go to the device) and cannot be captured into a graph; later calls
 * allocate nothing and can.
 * rt_scene_update_spheres: d_spheres holds count rt_sphere records in DEVICE memory; object_index in them is ignored.  Allocates
 * nothing; can be captured.
 * rt_scene_update_lights / _materials: count records in HOST memory, validated as rt_scene_create validates them (an unknown kind or
 * function: RT_ERR_INVALID_ARGUMENT, nothing written), staged in a pinned buffer the scene owns and copied from there on the stream.
 * The records are read at the call; a call waits for the copies of the call before it; on a stream that is being captured they are
 * RT_ERR_UNSUPPORTED. */
int rt_scene_update_vertices(rt_scene *scene, uint32_t first, uint32_t count, const rt_vertex *d_vertices, void *hip_stream);
int rt_scene_update_spheres(rt_scene *scene, uint32_t first, uint32_t count, const rt_sphere *d_spheres, void *hip_stream);
int rt_scene_update_lights(rt_scene *scene, uint32_t first, uint32_t count, const rt_light *h_lights, void *hip_stream);
int rt_scene_update_materials(rt_scene *scene, uint32_t first, uint32_t count, const rt_material *h_materials, void *hip_stream);

/* ---- motion queries: where a hit's point was before the scene update ------------------------------
 * What an animated sequence needs between a scene update and the temporal queries below: for each hit on the scene as it stands NOW,
 * the point of the same surface on the scene as it stood BEFORE the update — the plane of previous positions rt_temporal_motion
 * projects and rt_temporal_accumulate compares.  The scene keeps a snapshot (rt_scene_keep_positions), and a per-hit query carries a
 * hit point back onto it (rt_previous_positions).  Per frame: keep, then rt_scene_update_*, then cast, then rt_previous_positions.  The
 * hits must come from the scene as it stands now; the answer lies on the scene as it stood at the keep.  The reference has no
 * counterpart; the definition below is the contract.  It is written once (csrc/rt_motion.h) and compiled into both libraries without
 * contraction, so rt_previous_positions (any launch geometry), its _host form and rt_previous_positions_cpu (librt_host.so,
 * include/rt_host.h) return the same bits.
 *
 * rt_scene_keep_positions copies, into arrays the scene owns, the three vertex positions of every triangle and the centre and radius
 * of every sphere as they stand on the device at that point of hip_stream: "the kept positions".  Stream-ordered: an update put on the
 * same stream after it needs no synchronisation.  The first call on a scene allocates and is RT_ERR_UNSUPPORTED on a stream that is
 * being captured, as the first rt_scene_update_vertices is; later calls allocate nothing and can be captured.  The arrays are freed by
 * rt_scene_destroy; their layout is internal.  A scene with no triangles and no spheres is RT_OK, and afterwards counts as kept.  Each
 * keep replaces the one before.  rt_scene_positions_kept: 1 after a keep, 0 before; a null scene is RT_ERR_INVALID_ARGUMENT.
 *
 * rt_previous_positions writes, for record i, three f32 at d_was[i * was_stride + 0 .. 2]; other words of a wider stride are not
 * touched.  Every operation is a single f32 operation in the order written, none fused; dot(a, b) is (a0*b0 + a1*b1) + a2*b2 and
 * cross(a, b) is (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).  P = hit.position.
 *   TRIANGLE (kind == 1 and index < n_triangles), with v0, v1, v2, n, e0 = v2 - v1, e1 = v0 - v2, e2 = v1 - v0 and area the triangle's
 *   current values as rt_scene_create and rt_scene_update_vertices derive them, and q0, q1, q2 its kept vertices:
 *     1. m_k = q_k - v_k for k = 0, 1, 2
 *     2. if all nine components of m compare equal to zero, was = P, the raw words (a NaN keeps its payload, -0.0 stays -0.0): an
 *        unmoved triangle returns the hit position bit for bit, and the temporal queries on a scene where nothing moved give what they
 *        give without this block
 *     3. otherwise a0 = dot(cross(e0, P - v1), n), a1 = dot(cross(e1, P - v2), n), a2 = dot(cross(e2, P - v0), n) — the signed areas
 *        of the cast — and b_k = a_k / area: three divides, the barycentric weights of the hit
 *     4. was = P + ((m0 * b0 + m1 * b1) + m2 * b2) per component, each product rounded before its add
 *   NaN and Inf pass through the arithmetic; a moved degenerate triangle (area == 0) gives whatever the divides give.
 *   SPHERE (kind == 0 and index < n_spheres), with c, r the current centre and radius and cq, rq the kept ones: if cq == c in all three
 *   components and rq == r, was = P, the raw words; otherwise s = rq / r and was = cq + (P - c) * s.  rt_sphere has no orientation, so
 *   no rotation is modelled: a sphere that spins in place counts as unmoved.
 *   ANYTHING ELSE (RT_HIT_NONE, another kind, an index beyond its array): three words 0x7fc00000.  rt_temporal_motion then finds z > 0
 *   false and the pixel resets.
 * Checked before any device work, in this order: n >= 2^32 is RT_ERR_UNSUPPORTED; a null scene is RT_ERR_INVALID_ARGUMENT; a scene on
 * which rt_scene_keep_positions was never called is RT_ERR_INVALID_ARGUMENT (the message names that call); n == 0 is RT_OK and launches
 * nothing; a null pointer is RT_ERR_INVALID_ARGUMENT; was_stride < 3 is RT_ERR_INVALID_ARGUMENT.  ONE stream-ordered kernel launch on
 * hip_stream, one hit per lane; allocates nothing, visits the host for nothing and may be captured into a HIP graph at once.  It reads
 * the scene's arrays: ordering it after an update on another stream is the caller's business, as for a cast.
 * RT_AMD_DIAG_MOTION_MAX_GROUPS (rt_set_option): a test hook, both kernels launch at most this many workgroups and take the rest
 * grid-stride — same bits.
 * Not covered: the previous NORMAL of a rotating surface (the temporal normal test compares the current normal with the previous
 * frame's, and normal_min absorbs small rotations); motion of lights; rt_multi_* forms; tiles (rt_temporal_motion wants the full frame).
 * (A light that moved leaves no geometry to follow: what a history needs then is the colour-box clamp of the "history rectification
 * queries" below.) */
int rt_scene_keep_positions(rt_scene *scene, void *hip_stream);
int rt_scene_positions_kept(const rt_scene *scene); /* 1 / 0 */
int rt_previous_positions(const rt_scene *scene, const rt_hit *d_hits, size_t n, float *d_was, uint32_t was_stride, void *hip_stream);
/* The same kernel on HOST arrays: allocates, uploads the hits (and, for a stride above 3, the was plane, so that the words between the
 * records come back as they were), runs, synchronises the device and downloads.  NOT the CPU definition — that is
 * rt_previous_positions_cpu of librt_host.so. */
int rt_previous_positions_host(const rt_scene *scene, const rt_hit *h_hits, size_t n, float *h_was, uint32_t was_stride);

/* ---- several GPUs from one process (SURVEY §8e without Python or MPI) -------------------
 * Image rows are interleaved over the entries of `devices` exactly as homework-18-graphics-raytracer_amd/dist.py interleaves
 * them over ranks (entry r renders rows y0 + r*y_step, y0 + (r+n)*y_step, ...): the scene is replicated, the bands are
 * rendered concurrently, copied to pinned host memory and de-interleaved into the caller's image.  A device index may
 * repeat (several bands on one GPU).  This is the form a single-process host — the reference's main() — binds to use a
 * whole node; the one-process-per-GPU form over torch.distributed / RCCL is dist.py's.  Results are those of the
 * single-device entry points bit for bit: a pixel's value, and its random stream (seeded by IMAGE coordinates), do not
 * depend on which device renders it. */
typedef struct rt_multi rt_multi;
int rt_multi_create(const rt_scene_desc *desc, const int *devices, int n_devices, rt_multi **out);
int rt_multi_destroy(rt_multi *m);
/* rt_render_whitted_host over the devices: h_rgb = rt_frame_pixels(frame) * 3 floats; *h_ray_count = casts of all devices. */
int rt_multi_render_whitted_host(rt_multi *m, const rt_camera *camera, const rt_frame *frame, float *h_rgb, unsigned long long *h_ray_count);
/* rt_render_distributed_host over the devices.  The per-pixel generators live on the device that owns the pixel's row; they
 * are created on the first call for a frame and continue from call to call (main.rs:1131); a call with a different frame
 * starts new ones. */
int rt_multi_render_distributed_host(rt_multi *m, const rt_camera *camera, const rt_frame *frame, float focus, float blur, uint32_t n_epochs,
                                     float *h_accum, unsigned long long *h_ray_count);
/* The same two, device-resident: the frame is assembled in DEVICE memory on devices[0] (d_rgb / d_accum: rt_frame_pixels * 3
 * floats there; d_ray_count, may be NULL, a u64 there that the casts of all devices are ADDED to), so that
 * rt_post_process_device and rt_encode_srgb8_device can follow on `hip_stream` (a stream of devices[0]) without a trip
 * through host memory.  A band of another device travels by hipMemcpyPeerAsync (xGMI) into a staging buffer on devices[0]
 * and is de-interleaved there; no RCCL, no host bounce.  Asynchronous like rt_render_whitted: on return everything is
 * enqueued; work on `hip_stream` after the call sees the finished frame.  rt_multi_render_distributed continues from the
 * sums already in d_accum (main.rs:1165), exactly as rt_render_distributed does.  Replaces main.rs:1105-1109 / 1162-1167. */
int rt_multi_render_whitted(rt_multi *m, const rt_camera *camera, const rt_frame *frame, float *d_rgb, unsigned long long *d_ray_count, void *hip_stream);
int rt_multi_render_distributed(rt_multi *m, const rt_camera *camera, const rt_frame *frame, float focus, float blur, uint32_t n_epochs,
                                float *d_accum, unsigned long long *d_ray_count, void *hip_stream);

/* ---- the step after the path, on the device --------------------

 * post_process (src/main.rs:748-762): divide the image in place by the 99th-percentile luma of its normal
 * lumas (exact radix select; no sort).  *d_divisor (device float, may be NULL) receives the divisor used, 0 when
 * the image was left untouched (no normal luma, or percentile <= f32::EPSILON).  Bit-identical to
 * rt_post_process in librt_host.so.  Stream-ordered.  n_pixels = 0 is an image left untouched: nothing is read, and *d_divisor
 * (when not NULL) still receives 0 — by a write enqueued on hip_stream like every other, never from the host, so the call stays
 * asynchronous and can be captured (as rt_post_scale_device with n_pixels = 0, and as rt_post_process returns 0 for an empty
 * image; d_rgb may then be NULL).  d_divisor must be memory a device can reach; a pointer the runtime does not know as such is not written. */
int rt_post_process_device(float *d_rgb, size_t n_pixels, float *d_divisor, void *hip_stream);
/* rt_post_process_device keeps a grow-only scratch buffer per (device, stream); this frees those of the current device
 * (synchronises it first). */
int rt_post_release(void);
/* The same post_process for a frame whose row bands live on SEVERAL ranks or devices (src/main.rs:748-762 needs the 99th
 * percentile of ALL lumas): the passes of rt_post_process_device one by one on caller-owned device memory — d_keys: n_pixels
 * u32, d_state: RT_POST_STATE_WORDS u32 — so that the caller can sum d_state over the bands between them (an all-reduce on the
 * same stream order) and every band ends with the same divisor without a host round trip:
 *     rt_post_keys_device    zeroes d_state; one order-preserving key per pixel of THIS band; d_state[0] = its count of normal lumas
 *       -> sum d_state[0] over the bands
 *     for pass = 0 .. 3:
 *         rt_post_hist_device   d_state[4 .. 259] += histogram of this band's keys that match the digits chosen so far
 *           -> sum d_state[4 .. 259] over the bands
 *         rt_post_pick_device   every band picks the same digit from the same sums (and clears the histogram)
 *     rt_post_scale_device   divides this band by the selected luma (*d_divisor as for rt_post_process_device)
 * With one band and no sums in between this IS rt_post_process_device.  The k-th smallest does not depend on the order, so
 * the value equals the one main.rs:754 indexes after its sort.  Stream-ordered; n_pixels may be 0 (a rank without rows). */
#define RT_POST_STATE_WORDS 260
int rt_post_keys_device(const float *d_rgb, size_t n_pixels, uint32_t *d_keys, uint32_t *d_state, void *hip_stream);
int rt_post_hist_device(const uint32_t *d_keys, size_t n_pixels, int pass, uint32_t *d_state, void *hip_stream);
int rt_post_pick_device(int pass, uint32_t *d_state, void *hip_stream);
int rt_post_scale_device(float *d_rgb, size_t n_pixels, const uint32_t *d_state, float *d_divisor, void *hip_stream);
/* Image::<Srgb<u8>>::convert_from (src/image.rs:55-66): linear f32 -> sRGB-encoded u8, n_values = 3*pixels. */
int rt_encode_srgb8_device(const float *d_rgb, size_t n_values, unsigned char *d_out, void *hip_stream);
/* PhotonAccumulator (src/photon.rs:9-34; unused by the reference's main()) on the device, bit-identical to
 * rt_accumulate / rt_accumulator_resolve in librt_host.so: d_sum (3 f32 per pixel) and d_weight (1 f32 per pixel) start
 * at zero; rt_accumulate_device applies accumulate() for every sample whose filter flag is set (d_samples, d_valid: the
 * n_epochs x n_pixels outputs of rt_render_distributed), in epoch order; rt_accumulator_resolve_device writes
 * sum / weight, black while weight < f32::EPSILON.  Stream-ordered.  n_epochs = 0 or n_pixels = 0 changes nothing, and the arrays
 * such a call would not read (d_samples and d_valid without epochs, all four without pixels) may be NULL. */
int rt_accumulate_device(const float *d_samples, const unsigned char *d_valid, uint32_t n_epochs, size_t n_pixels, float *d_sum,
                         float *d_weight, void *hip_stream);
int rt_accumulator_resolve_device(const float *d_sum, const float *d_weight, size_t n_pixels, float *d_rgb, void *hip_stream);

/* ---- bloom queries: the highlight bloom post_process leaves as a TODO ------------------------------

 * The reference's post_process ends with "TODO: highlight bloom effect".  rt_post_process_device divides by the 99th-percentile luma, so
 * about one pixel in a hundred ends above 1.0 and rt_encode_srgb8_device clips it flat: lamp reflections and specular peaks become hard
 * white blobs.  Bloom spreads what lies above a threshold over its surroundings before the encode, the one step between the two:
 *     ... -> rt_post_process_device -> rt_bloom -> rt_encode_srgb8_device
 * The reference has no counterpart; the definition below is the contract.  It is written once (csrc/rt_bloom.h) and compiled into both
 * libraries without contraction, so the device form (either kernel form, any launch geometry), the _host form and rt_bloom_cpu
 * (librt_host.so, include/rt_host.h) return the same bits.  The device call is 2 L stream-ordered kernel launches on hip_stream and
 * nothing else — L down launches (the first fused with the bright pass), L - 1 up-and-add launches, one composite —, allocates nothing,
 * visits the host for nothing and may be captured into a HIP graph at once.  Every output word is written by one thread: no atomics,
 * nothing depends on the launch.
 *
 * color is a plane as in the denoise queries: a base pointer and a pixel stride in 4-byte WORDS (>= 3), pixel i = r * cols + c, so the
 * colour inside rt_temporal_pixel records (stride 8) is read where it lies.  out: 3 f32 per pixel, compact; it may be color itself when
 * color_stride == 3 (the composite reads a pixel's colour only at that pixel).  temp: opaque scratch of rt_bloom_temp_bytes bytes.
 * Every operation is a single f32 operation in the order written, none fused; the divide is correctly rounded.  Level sizes:
 * rows_0 = rows, rows_j = ceil(rows_{j-1} / 2), the same for columns; a level may be 1 x 1, and the level after it is 1 x 1 again.
 * L = n_levels; clamp(i, n) puts an index into 0 .. n - 1.
 *   1. bright pass: at a level-0 pixel with colour c,  l = (w0 * c_r + w1 * c_g) + w2 * c_b  with post_process's luma row (computed on the
 *      host, as rt_post_process_device gets it).  If any channel has c - c != 0 (not finite), or !(l > 0):  B = (+0, +0, +0) — the
 *      reference's is_normal filters keep such pixels out of its sums; here they are kept from spreading.  Otherwise  s = l - threshold;
 *      with knee > 0:  t = fminf(fmaxf(s + knee, 0), 2 * knee);   q = (t * t) / (4 * knee);   m = fmaxf(s, q);   with knee == 0:  m = s.
 *      If !(m > 0):  B = +0;  otherwise  B_k = c_k * (m / l).
 *   2. down: for j = 1 .. L, D_j(r, c) from the source S = B (j = 1) or D_{j-1}: source rows clamp(2 r - 1 + kr), columns
 *      clamp(2 c - 1 + kc), kr, kc = 0 .. 3;  per source row  h_kr = (s_0 + 3 * s_1) + (3 * s_2 + s_3);   then
 *      D = ((h_0 + 3 * h_1) + (3 * h_2 + h_3)) * (1 / 64),  per channel: the [1 3 3 1] / 8 tent centred on the 2 x 2 block with replicated
 *      edges, so a constant stays a constant at every border and every odd size.
 *   3. up and add: U_L = D_L; for j = L - 1 .. 1,  U_j(r, c) = D_j(r, c) + up(U_{j+1})(r, c),  written over D_j in place, where
 *      up(X)(r, c):  near_r = r >> 1;   far_r = clamp(near_r + (r odd ? 1 : -1));  the same for columns;
 *      h_near = 3 * X(near_r, near_c) + X(near_r, far_c);   h_far likewise on row far_r;   up = (3 * h_near + h_far) * (1 / 16).
 *   4. composite:  g = intensity / (float)L, computed once on the host;   out_k = c_k + g * up(U_1)_k.  A colour that is not finite stays
 *      whatever c_k + ... gives; it glows nowhere else (step 1).
 *   5. temp holds D_1 .. D_L compact, one after the other: rt_bloom_temp_bytes = sum over j = 1 .. L of rows_j * cols_j * 12, and 0 for
 *      an n_levels that is refused.
 * Consequences: threshold = +inf or intensity = 0 returns the colour's values; the tap sums are mirror-symmetric, so on a size that is
 * a multiple of 2^L both ways a mirrored image gives the mirrored result, bit for bit.
 *
 * Checked before any device work, all RT_ERR_INVALID_ARGUMENT with a message that names the argument, in this order: a null params;
 * n_levels outside 1 .. RT_BLOOM_MAX_LEVELS; a threshold that is NaN or negative (+inf is legal: nothing glows); a knee that is NaN,
 * negative or infinite; an intensity that is NaN, negative or infinite; color_stride < 3; rows * cols >= 2^32; then rows == 0 or
 * cols == 0 is RT_OK and launches nothing; a null color, out or (where the form takes it: not rt_bloom_host, whose round trip makes
 * its own) temp; out == color with color_stride != 3.
 * RT_AMD_BLOOM_FORM (rt_set_option): 0 every step the plain kernel, every tap read from global memory; 1 the down steps the tiled
 * kernel, a workgroup's 34 x 34 sources staged in LDS once, after the bright pass; same bits (DESIGN.md 3.30 says which is the default
 * and why).  RT_AMD_DIAG_BLOOM_MAX_GROUPS: a test hook, a step launches at most this many workgroups and takes the rest of its level
 * grid-stride; same bits.
 * Not covered: the rt_multi_* sharded finish (a band's bloom needs its neighbours' rows); lens dirt and anamorphic kernels; tone
 * mapping other than post_process's divide; rt_render, which gets no flag. */

#define RT_BLOOM_MAX_LEVELS 8u

typedef struct rt_bloom_params {
    float threshold;    /* luma above which a pixel glows; +inf: nothing does */
    float knee;         /* half-width of the soft transition around threshold; 0: a hard cut */
    float intensity;    /* weight of the whole bloom in the composite */
    uint32_t n_levels;  /* 1 .. RT_BLOOM_MAX_LEVELS (8) */
} rt_bloom_params;      /* 16 bytes */

/* the bytes of d_temp for an image of rows x cols at n_levels (step 5); host arithmetic, 0 for an n_levels outside 1 .. 8 */
size_t rt_bloom_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels);
/* d_color: rows * cols pixels of 3 f32 at color_stride words; d_temp: rt_bloom_temp_bytes bytes; d_out: rows * cols * 3 f32, or d_color
 * itself when color_stride == 3; 2 n_levels kernel launches.  Nothing but d_temp and d_out is written. */
int rt_bloom(const float *d_color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *d_temp,
             float *d_out, void *hip_stream);
/* The same kernels on HOST arrays: allocate, upload the colour with its stride, run, synchronise the device and download.  h_temp is
 * not looked at (it may be NULL): the round trip makes the scratch on the device.  NOT the CPU definition — that is rt_bloom_cpu of
 * librt_host.so. */
int rt_bloom_host(const float *h_color, uint32_t color_stride, const rt_bloom_params *params, uint32_t rows, uint32_t cols, float *h_temp,
                  float *h_out);

/* ---- film queries: sub-pixel camera rays and filtered accumulation ------------------------------

 * The image side of the per-pixel loop: where in its pixel a sample is taken, the primary ray through that position, and what a sample
 * adds to the pixels around it — PhotonAccumulator::accumulate_weight (photon.rs:30-33: sum = sum + photon * weight; weight_sum +=
 * weight), which the reference defines and never calls, behind a reconstruction filter.  With rt_trace_rays or
 * rt_trace_rays_distributed in between this is a supersampled, antialiased frame:
 *     rt_film_offsets -> rt_camera_rays_offset -> rt_trace_rays -> rt_film_splat -> rt_accumulator_resolve_device
 * All buffers are SAMPLE-MAJOR: sample s of compact pixel i is record s * n_pixels + i, the (n_epochs, n_pixels) layout of
 * rt_accumulate_device and rt_trace_rays_distributed.  Every pointer is a device pointer; every call is stream-ordered and asynchronous
 * on hip_stream (NULL = default stream), allocates nothing, visits the host for nothing, uses no workspace and may be captured into a HIP
 * graph at once.  The splat is a GATHER in a fixed order — no atomics — so a result does not change from run to run, does not depend on
 * the launch geometry, and is bit-identical to the host forms rt_film_offsets_host / rt_film_splat_host of librt_host.so
 * (include/rt_host.h), which are the CPU definition.
 * Not covered: halos between the bands of a frame that is spread over several ranks — the image of rt_film_splat is ONE compact
 * rows x cols array, and samples beyond its edge do not exist; rt_multi_* forms. */

#define RT_FILM_CENTER 0u     /* every offset (+0, +0): the pixel's integer coordinate, as rt_camera_rays */
#define RT_FILM_UNIFORM 1u    /* any spp: offset = u - 0.5f */
#define RT_FILM_STRATIFIED 2u /* spp = k * k, 1 <= k <= 8: sample s in cell (s % k, s / k), offset = ((float)cell + u) / (float)k - 0.5f */

#define RT_FILM_BOX 0u
#define RT_FILM_TENT 1u
#define RT_FILM_MITCHELL 2u

/* d_offsets[2 * (s * n_pixels + i) + axis] (axis 0: dx, 1: dy, in pixels) for the spp samples of every pixel of a frame or tile, in its
 * compact row order.  u is a counter hash of the GLOBAL pixel index pixel = y * width + x (u32, not the compact index: the tiles of a
 * sharded frame agree with each other and with the full frame), all in u32 arithmetic:
 *     mix(v):  v ^= v >> 16;  v *= 0x7feb352d;  v ^= v >> 15;  v *= 0x846ca68b;  v ^= v >> 16
 *     h = mix(mix(pixel + seed) ^ (2 * s + axis));   u = (float)(h >> 8) * 2^-24        (0 <= u < 1)
 * so every offset lies in [-0.5, 0.5].  frame->max_depth is not used.
 * Checked before any device work, in this order: a null frame, a bad frame, spp == 0, an unknown pattern, a stratified spp that is no
 * k * k with 1 <= k <= 8: RT_ERR_INVALID_ARGUMENT; 2^32 samples or more: RT_ERR_UNSUPPORTED; a null d_offsets: RT_ERR_INVALID_ARGUMENT. */
int rt_film_offsets(const rt_frame *frame, uint32_t spp, uint32_t pattern, uint32_t seed, float *d_offsets, void *hip_stream);

/* Camera::shoot through (x + dx, y + dy): d_rays[s * n_pixels + i] for the offsets d_offsets[2 * (s * n_pixels + i) ..] (rt_film_offsets, or
 * the caller's own), with
 *     clip_y = (half_height - ((float)y + dy)) / height_f;     clip_x = (((float)x + dx) - half_width) / height_f
 * and everything after that in rt_camera_rays' operations (one function serves both); records as rt_camera_rays writes them.  With all
 * offsets +0 the output is rt_camera_rays' byte for byte, spp times.  Tiles and y_step as in rt_camera_rays; frame->max_depth is not used.
 * Checked in this order: a null camera or frame, a bad frame, spp == 0: RT_ERR_INVALID_ARGUMENT; 2^32 rays or more: RT_ERR_UNSUPPORTED; a
 * null pointer: RT_ERR_INVALID_ARGUMENT. */
int rt_camera_rays_offset(const rt_camera *camera, const rt_frame *frame, const float *d_offsets, uint32_t spp, rt_ray *d_rays, void *hip_stream);
/* The same on HOST arrays: allocates, copies, runs, synchronises the device and copies back. */
int rt_camera_rays_offset_host(const rt_camera *camera, const rt_frame *frame, const float *h_offsets, uint32_t spp, rt_ray *h_rays);

/* accumulate_weight with a reconstruction filter, over a compact image of rows x cols pixels (n_pixels = rows * cols):
 *     d_samples  3 f32 per sample          d_valid   1 u8 per sample, NULL: every sample counts
 *     d_offsets  2 f32 per sample          d_sum     3 f32 per pixel, d_weight 1 f32 per pixel: READ, UPDATED AND WRITTEN — what
 *                                                    PhotonAccumulator holds and rt_accumulator_resolve_device resolves; start them at zero
 * For output pixel (r, c), with reach = (int)ceilf(radius + 0.5f):
 *     for s = 0 .. spp - 1:                          (outermost)
 *       for dr = -reach .. reach:  for dc = -reach .. reach:          (ascending)
 *         q = (r + dr, c + dc); skipped when outside the image or when d_valid[s * n_pixels + q] == 0
 *         ddx = (float)dc + dx_q;   ddy = (float)dr + dy_q                   (q's offset of sample s)
 *         contributes only if  -radius <= ddx < radius  and  -radius <= ddy < radius      (half-open)
 *         w = f(ddx) * f(ddy);   sum_c = sum_c + photon_c * w  (c = 0, 1, 2; the product is rounded, then added);   weight = weight + w
 * with the filter f(d), every operation a single f32 operation in the order written, none fused:
 *     RT_FILM_BOX       1.0f
 *     RT_FILM_TENT      1.0f - fabsf(d) / radius
 *     RT_FILM_MITCHELL  (Mitchell-Netravali, B = C = 1/3)   x = 2.0f * fabsf(d) / radius
 *                       x < 1:      ((7.0f * x - 12.0f) * x * x + 16.0f / 3.0f) / 6.0f
 *                       otherwise:  (((-7.0f / 3.0f * x + 12.0f) * x - 20.0f) * x + 32.0f / 3.0f) / 6.0f
 *                       (16.0f / 3.0f, -7.0f / 3.0f and 32.0f / 3.0f are f32 constants; -7.0f / 3.0f * x is (-7.0f / 3.0f) * x)
 * Consequences: a box of radius 0.5 with offsets in [-0.5, 0.5) gives every sample to its own pixel with w == 1, and the call is
 * rt_accumulate_device bit for bit; because s is outermost, one call with spp samples equals spp calls with one sample each (progressive
 * accumulation); nothing depends on how the kernel is launched.  An offset outside [-0.5, 0.5] is legal, NaN included: the sample simply
 * does not reach every pixel its filter covers (only the (2 reach + 1)^2 pixels around its own are looked at), a NaN offset reaches none.
 * A NaN or Inf sample value passes through the arithmetic into the pixels it contributes to, and only those.
 * Checked before any device work: an unknown filter, a radius outside 0 < radius <= 4, spp == 0, rows * cols >= 2^32, a null pointer
 * (other than d_valid): all RT_ERR_INVALID_ARGUMENT.  rows == 0 or cols == 0 is RT_OK and launches nothing. */
int rt_film_splat(uint32_t rows, uint32_t cols, const float *d_samples, const unsigned char *d_valid, const float *d_offsets, uint32_t spp,
                  uint32_t filter, float radius, float *d_sum, float *d_weight, void *hip_stream);

/* ---- adaptive sampling queries: sample budgets, lists and listed splats ----------------------------

 * What turns a variance estimate into more samples where they are needed.  The film queries above take ONE spp for the whole frame and
 * are sample-major; these five calls are their ragged counterpart, PIXEL-MAJOR: a budget per pixel (rt_sample_budget), the list of the
 * samples it asks for (rt_sample_list), and the film queries on that list:
 *     rt_sample_budget -> rt_sample_list -> rt_film_offsets_listed -> rt_camera_rays_listed -> rt_trace_rays -> rt_film_splat_listed
 * The reference has no counterpart; the definitions below are the contract.  The arithmetic is written once (csrc/rt_adaptive.h, on
 * csrc/rt_film.h's film_u / film_offset / film_reach / film_covers / film_apply, unchanged) and compiled into both libraries without
 * contraction, so the device forms (any launch geometry, either splat form) and rt_sample_budget_cpu / rt_sample_list_cpu /
 * rt_film_offsets_listed_cpu / rt_camera_rays_listed_cpu / rt_film_splat_listed_cpu (librt_host.so, include/rt_host.h) return the same
 * bits.  Every pointer is a device pointer; every call is stream-ordered and asynchronous on hip_stream (NULL = default stream),
 * allocates nothing, visits the host for nothing — the number of listed records stays on the device, in d_total — and may be captured
 * into a HIP graph at once, the first call on a stream included: the only scratch is the caller's d_temp.  Every output word is written
 * by one thread; no atomics; record numbers are counted in 64 bits.  Every f32 operation is a single operation in the order written, none
 * fused; divide and square root are correctly rounded.
 *
 * rt_sample_budget, for pixel p of n.  mean, variance (f32) and count, valid (u32) are planes of one word per pixel read through record
 * strides given in 4-byte words, so moment1 and length inside rt_temporal_pixel records are read with stride 8 and no copy, beside a
 * compact variance plane (rt_temporal_accumulate's d_variance, rt_svgf_variance).  count NULL is 1 everywhere; valid NULL is "all".
 *   1. valid given and valid_p == 0:  budget_p = 0
 *   2. count_p == 0 (no estimate):   budget_p = max_count
 *   3. e = sqrtf(variance_p / (float)count_p) / (fabsf(mean_p) + epsilon)        the relative standard error of the mean
 *   4. t = e * gain
 *   5. range = max_count - min_count
 *   6. budget_p = min_count + (t < (float)range ? (uint32_t)t : range)
 * The float test comes before the conversion, so a NaN or a huge t gives max_count and is never converted.  A negative variance gives a
 * NaN under the root and therefore max_count; so do a NaN variance, a NaN mean and +inf variance.  Variance 0 or gain 0 gives min_count
 * (gain 0 with an infinite e is 0 * inf = NaN: max_count).  d_budget is a compact u32 plane.  One element-wise kernel, grid-stride.
 * Checked before any device work, in this order, RT_ERR_INVALID_ARGUMENT unless said: n >= 2^32 (RT_ERR_UNSUPPORTED); n == 0 is RT_OK and
 * launches nothing; a null params; a null mean, variance or budget; a stride of 0 words; gain >= 0 false; epsilon > 0 false;
 * min_count <= max_count <= RT_SAMPLE_MAX false; flags != 0.
 * Normalising the budgets to a fixed total is not part of it: the total comes out of rt_sample_list on the device, and a caller adjusts
 * gain from it.
 *
 * rt_sample_list.  c_i = min(d_counts[i], RT_SAMPLE_MAX) — the caller's counts are validated, never trusted — and S_i = c_0 + .. + c_(i-1)
 * (S_0 = 0), all below 2^32 because n * RT_SAMPLE_MAX < 2^32 is required.
 *   start_i = min(S_i, capacity)                                   for i = 0 .. n                     d_start[n + 1]
 *   for start_i <= j < start_(i+1):  pixel[j] = i,  sample[j] = first_i + (j - start_i)                d_pixel, d_sample[capacity]
 *   d_total[0] = start_n  (the records listed);   d_total[1] = S_n  (the records asked for: larger only when the list was cut)
 *   first_i = 0 when d_first is NULL; with d_first (n words, in and out) afterwards  first_i += start_(i+1) - start_i,  so a progressive
 *   caller never repeats a sample index
 * A pixel that straddles capacity keeps its first samples.  Entries of d_pixel / d_sample at and beyond d_total[0] are unspecified.  The
 * list is pixel-major on purpose: the samples of one pixel, and of neighbouring pixels, are adjacent, so 64 consecutive rays stay
 * coherent.  Three kernel launches: per-step totals, a one-workgroup scan, placement and expansion — integer sums only, so nothing depends
 * on the launch geometry.  d_temp: rt_sample_list_temp_bytes(n) bytes of opaque scratch, 4-byte aligned (host arithmetic, monotone in n,
 * 0 for n == 0 and for an n the call refuses).
 * Checked before any device work, in this order: n * RT_SAMPLE_MAX >= 2^32, then capacity >= 2^32 (RT_ERR_UNSUPPORTED); a null start or
 * total; n == 0 is RT_OK, writes start_0 = 0 and both totals 0 and launches nothing else; a null counts; capacity != 0 and a null pixel or
 * sample; a temp that is null, too small or misaligned (all RT_ERR_INVALID_ARGUMENT).
 *
 * rt_film_offsets_listed.  listed = min(d_total[0], capacity).  For j < listed with pixel[j] < rows * cols of the frame or tile:
 *   offsets[2 j + axis] = film_offset(pattern, global pixel, seed, sample[j], axis)      (rt_film_offsets' hash, keyed by the GLOBAL index
 *   (y0 + row * y_step) * width + (x0 + col) of compact pixel pixel[j] = row * cols + col)
 * so sample s of a pixel has the offset rt_film_offsets gives sample s of that pixel.  RT_FILM_CENTER and RT_FILM_UNIFORM only:
 * RT_FILM_STRATIFIED is RT_ERR_INVALID_ARGUMENT (a ragged pass has no k x k).  Every other record of [0, capacity) — from listed on, or of
 * a pixel the frame does not have — gets NaN for both offsets; a NaN dx is covered by no one, as in rt_film_splat.
 * Checked in this order: a null frame; a bad frame; a stratified, then an unknown pattern; 2^32 pixels or capacity >= 2^32
 * (RT_ERR_UNSUPPORTED); capacity == 0 is RT_OK and launches nothing; a null pointer.
 *
 * rt_camera_rays_listed.  For j < listed with pixel[j] in range: rays[j] = rt_camera_rays_offset's record of that pixel through
 * (x + offsets[2 j], y + offsets[2 j + 1]) (one function serves both).  Every other record of [0, capacity) is the all-zero ray — the
 * record rt_tree_gather writes for an absent candidate — so a fixed-size rt_trace_rays(capacity) in a captured graph is defined; what
 * it returns for those records is never read by rt_film_splat_listed.  Checked in this order: a null camera or frame; a bad frame; 2^32
 * pixels or capacity >= 2^32 (RT_ERR_UNSUPPORTED); capacity == 0 is RT_OK; a null pointer.
 *
 * rt_film_splat_listed: rt_film_splat on a list.  d_samples (3 f32), d_valid (1 u8, or NULL), d_offsets (2 f32) hold one record per
 * listed sample, [0, capacity); d_start is rt_sample_list's; max_count (1 .. RT_SAMPLE_MAX) is the host's bound on a pixel's count.
 * With lo_q = min(start_q, capacity), hi_q = min(start_(q+1), capacity) and count_q = hi_q > lo_q ? hi_q - lo_q : 0 — so a d_start that
 * decreases or exceeds capacity never causes a read outside [0, capacity) — for output pixel (r, c), reach = (int)ceilf(radius + 0.5f):
 *     for s = 0 .. max_count - 1:                    (outermost)
 *       for dr = -reach .. reach:  for dc = -reach .. reach:          (ascending)
 *         q = (r + dr, c + dc); skipped when outside the image, when s >= count_q, or when d_valid[lo_q + s] == 0
 *         then rt_film_splat's support test, weight and sums on record lo_q + s
 * d_sum and d_weight are read, updated and written in place by one thread per output pixel.  Samples of a pixel beyond max_count are not
 * applied.  Two kernel forms, the plain gather and a 16 x 16 LDS tile that skips an s no pixel of its halo has, chosen by
 * RT_AMD_FILM_SPLAT_FORM as for rt_film_splat: same bits.
 * Consequences: with every count equal to spp the result is rt_film_splat's bit for bit (the records are the same samples, merely laid
 * out pixel-major); with a box of radius 0.5, centre offsets and count 1 it is rt_accumulate_device's.
 * Checked in this order: an unknown filter; a radius outside 0 < radius <= 4; max_count outside 1 .. RT_SAMPLE_MAX (RT_ERR_INVALID_ARGUMENT);
 * rows * cols >= 2^32 or capacity >= 2^32 (RT_ERR_UNSUPPORTED); rows == 0 or cols == 0 is RT_OK and launches nothing; a null start, sum or
 * weight; capacity != 0 and a null sample or offset pointer.
 * RT_AMD_DIAG_ADAPTIVE_MAX_GROUPS (rt_set_option): a test hook, every kernel of this block launches at most this many workgroups and takes
 * the rest grid-stride; same bits.
 * Not covered: banded frames and rt_multi_* forms; stratified or low-discrepancy ragged patterns; a budget normalised to a fixed total;
 * _host forms (host buffers through the device); adaptive depth-of-field epochs, whose generators are per pixel, not per sample. */

#define RT_SAMPLE_MAX 64u    /* the most samples one pixel may take in one list */

typedef struct rt_sample_budget_params {
    float gain;               /* samples per unit of relative standard error; >= 0 */
    float epsilon;            /* added to |mean|; > 0 */
    uint32_t min_count;       /* min_count <= max_count <= RT_SAMPLE_MAX */
    uint32_t max_count;
    uint32_t flags;           /* reserved: 0 */
} rt_sample_budget_params;   /* 20 bytes */

int rt_sample_budget(const float *d_mean, uint32_t mean_stride, const float *d_variance, uint32_t variance_stride,
                     const uint32_t *d_count /* or NULL */, uint32_t count_stride, const uint32_t *d_valid /* or NULL */, uint32_t valid_stride,
                     const rt_sample_budget_params *params, size_t n, uint32_t *d_budget, void *hip_stream);
size_t rt_sample_list_temp_bytes(size_t n);
int rt_sample_list(const uint32_t *d_counts, size_t n, size_t capacity, uint32_t *d_first /* or NULL */, uint32_t *d_start, uint32_t *d_pixel,
                   uint32_t *d_sample, uint32_t *d_total, void *d_temp, size_t temp_bytes, void *hip_stream);
int rt_film_offsets_listed(const rt_frame *frame, uint32_t pattern, uint32_t seed, const uint32_t *d_pixel, const uint32_t *d_sample,
                           const uint32_t *d_total, size_t capacity, float *d_offsets, void *hip_stream);
int rt_camera_rays_listed(const rt_camera *camera, const rt_frame *frame, const float *d_offsets, const uint32_t *d_pixel, const uint32_t *d_total,
                          size_t capacity, rt_ray *d_rays, void *hip_stream);
int rt_film_splat_listed(uint32_t rows, uint32_t cols, const float *d_samples, const unsigned char *d_valid, const float *d_offsets,
                         const uint32_t *d_start, size_t capacity, uint32_t max_count, uint32_t filter, float radius, float *d_sum,
                         float *d_weight, void *hip_stream);

/* ---- denoise queries: an edge-avoiding A-Trous filter on guide planes ------------------------------

 * What turns the noisy image of a few stochastic epochs into a clean one on the device: the edge-avoiding A-Trous wavelet filter
 * (Dammertz, Sewtz, Hanika, Lensch: "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG 2010), one
 * level per kernel launch, guided by the planes rt_material_hits already produces (shading normal, position, albedo, valid):
 *     rt_render_distributed / rt_film_splat -> resolve -> rt_camera_rays -> rt_cast_rays -> rt_material_hits -> rt_denoise_atrous -> rt_post_process_device
 * The reference has no denoiser; the definition below is the contract.  It is written once (csrc/rt_denoise.h) and compiled into both
 * libraries without contraction, so rt_denoise_atrous (both kernel forms, any launch geometry), rt_denoise_atrous_host and
 * rt_denoise_atrous_cpu (librt_host.so, include/rt_host.h) return the same bits.  Every device call is stream-ordered and asynchronous on
 * hip_stream, allocates nothing, visits the host for nothing, and may be captured into a HIP graph at once.  Each output pixel is written
 * by one thread, which walks its 25 sources in a fixed order: no atomics, nothing depends on the launch.
 *
 * The image is ONE compact array of rows x cols pixels, 3 f32 each, pixel i = r * cols + c.  A guide plane is a base pointer and a
 * record stride in 4-byte WORDS: pixel i's values are base[i * stride + 0 .. width - 1] (width 3 for normal, position and albedo, 1 for
 * valid), so the fields of rt_hit (13 words) and rt_surface (18 words) records are passed where they lie — e.g. position =
 * (const float *)hits + 3, stride 13; normal = (const float *)surfaces + 14, albedo = (const float *)surfaces + 3, valid =
 * (const uint32_t *)surfaces + 17, stride 18.  Stride 3 (1 for valid) is the compact plane.  Any guide pointer may be NULL: that term of
 * the exponent is left out / every pixel is valid.
 *
 * One level l (0 <= l <= 5), step s = 1 << l, input plane `in`, for output pixel p = (r, c); every operation is a single f32 operation
 * in the order written, none fused, unless it says binary64:
 *   1. the colour seen at a pixel q:  C_q[k] = in[3 q + k];  when the level demodulates its input, C_q[k] = in[3 q + k] / (albedo_q[k] + 1e-3f)
 *   2. p passes through — out[3 p + k] = in[3 p + k], the raw words, no other arithmetic — when valid is not NULL and valid_p == 0
 *   3. otherwise sum_0 = sum_1 = sum_2 = wsum = +0, and for dr = -2 .. 2 (outer), dc = -2 .. 2 (inner), both ascending:
 *        q = (r + dr * s, c + dc * s);  skipped when outside the image, or when valid is not NULL and valid_q == 0
 *        dist2(a, b):  d_k = a[k] - b[k];  (d_0 * d_0 + d_1 * d_1) + d_2 * d_2
 *        x = dist2(C_p, C_q) / sc2;   if normal:  x = x + dist2(n_p, n_q) / sn2;   if position:  x = x + dist2(P_p, P_q) / sp2
 *            where sc = sigma_color * 2^-(l - first_level) (an exact multiply by a power of two), sc2 = sc * sc,
 *            sn2 = sigma_normal * sigma_normal, sp2 = sigma_position * sigma_position;  a sigma of +inf makes its term +0
 *        skipped unless x >= 0  (so a NaN x — a NaN colour or guide on either side — skips the tap)
 *        e = x > 100 ? +0 : (float)rtdm::exp_mid(-(double)x)     binary64 exponential of csrc/rt_detmath.h (+ - * / only), rounded once
 *        w = h[dr + 2] * h[dc + 2] * e                           h = {1/16, 1/4, 3/8, 1/4, 1/16}, the B3 spline, exact in f32
 *        sum_k = sum_k + C_q[k] * w  (the product rounded, then added; k = 0, 1, 2);   wsum = wsum + w
 *   4. if wsum > 0:  out[3 p + k] = sum_k / wsum, times (albedo_p[k] + 1e-3f) when the level remodulates its output;
 *      otherwise (a NaN centre colour, for one) p passes through as in 2.
 * A tap with x > 100 still takes part, with w = +0: it changes nothing unless C_q is infinite (Inf * 0 = NaN) — mark such pixels invalid.
 *
 * A call runs levels first_level .. first_level + n_levels - 1, each reading the previous one's output; the planes alternate between
 * d_out and d_temp so that the LAST level writes d_out; d_color is only read.  flags: RT_DENOISE_DEMODULATE_IN makes the call's first
 * level demodulate its input (step 1), RT_DENOISE_DEMODULATE_OUT makes its last level remodulate its output (step 4);
 * RT_DENOISE_DEMODULATE is both — the filter then works on irradiance and leaves texture detail alone.  The levels in between work on what
 * the previous level wrote.  Consequence: one call of n levels equals n calls of one level each, level j (0-based) of them with
 * first_level + j, sigma_color * 2^-j (sigma_color is the sigma of the CALL's first level), and DEMODULATE_IN on the first call only,
 * DEMODULATE_OUT on the last only.
 * Checked before any device work, all RT_ERR_INVALID_ARGUMENT with a message that names the argument: a null guides or params; rows * cols
 * >= 2^32; n_levels < 1 or first_level + n_levels > 6; a sigma that is not > 0 (NaN included; +inf is legal); unknown flag bits; a
 * demodulation flag without an albedo plane; a stride smaller than its plane's width; a null d_color or d_out; a null d_temp with
 * n_levels >= 2; d_out or d_temp equal to d_color or to each other.  rows == 0 or cols == 0 is RT_OK and launches nothing.
 * Not covered here: variance-guided sigmas — they are rt_svgf_atrous of the "variance-guided filter queries" below; temporal accumulation
 * — the "temporal queries" below; halos between the bands of a sharded frame (pixels beyond the edge of the array do not exist),
 * rt_multi_* forms. */

#define RT_DENOISE_DEMODULATE_IN 1u
#define RT_DENOISE_DEMODULATE_OUT 2u
#define RT_DENOISE_DEMODULATE 3u
#define RT_DENOISE_MAX_LEVELS 6u

typedef struct rt_denoise_guides {
    const float *normal;      /* 3 f32 per pixel, or NULL */
    const float *position;    /* 3 f32 per pixel, or NULL */
    const float *albedo;      /* 3 f32 per pixel, or NULL; needed by the demodulation flags only */
    const uint32_t *valid;    /* 1 word per pixel, 0: the pixel is neither filtered nor a source; or NULL */
    uint32_t normal_stride;   /* record strides in 4-byte words: >= 3 ... */
    uint32_t position_stride;
    uint32_t albedo_stride;
    uint32_t valid_stride;    /* ... >= 1; the stride of a NULL plane is not looked at */
} rt_denoise_guides;         /* 48 bytes */

typedef struct rt_denoise_params {
    float sigma_color;        /* of the call's first level; halves with every further level */
    float sigma_normal;
    float sigma_position;     /* each > 0, +inf: the term is off */
    uint32_t first_level;
    uint32_t n_levels;        /* first_level + n_levels <= RT_DENOISE_MAX_LEVELS */
    uint32_t flags;           /* RT_DENOISE_DEMODULATE_* */
} rt_denoise_params;         /* 24 bytes */

/* what d_temp of rt_denoise_atrous must hold: one colour plane, rows * cols * 12 bytes (no guide is repacked) */
size_t rt_denoise_temp_bytes(uint32_t rows, uint32_t cols);
/* d_color, d_out, d_temp: rows * cols * 3 f32 on the device, three different buffers; one kernel launch per level */
int rt_denoise_atrous(const float *d_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                      float *d_out, float *d_temp, void *hip_stream);
/* The same kernels on HOST arrays (the pointers of `guides` are host pointers too): allocates, uploads every plane with its stride,
 * runs, synchronises the device and downloads h_out.  No h_temp: the round trip makes its own.  NOT the CPU definition — that is
 * rt_denoise_atrous_cpu of librt_host.so, which needs no device; this one is how a caller without device buffers runs the kernels. */
int rt_denoise_atrous_host(const float *h_color, const rt_denoise_guides *guides, const rt_denoise_params *params, uint32_t rows, uint32_t cols,
                           float *h_out);

/* ---- temporal queries: reprojected history with luminance moments --------------------------------

 * What lies between two frames of a sequence: where each pixel's surface point was in the previous frame (rt_temporal_motion), and the
 * previous frame's accumulated colour gathered from there and blended with the current one, with the first two moments of luminance
 * (rt_temporal_accumulate) — the temporal half of Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017):
 *     ... resolve -> rt_camera_rays -> rt_cast_rays -> rt_material_hits -> rt_temporal_motion -> rt_temporal_accumulate -> rt_denoise_atrous -> rt_post_process_device
 * The reference has no counterpart; the definition below is the contract.  It is written once (csrc/rt_temporal.h) and compiled into
 * both libraries without contraction, with no libm call and no device intrinsic, so rt_temporal_motion / rt_temporal_accumulate (any
 * launch geometry), their _host forms and rt_temporal_motion_cpu / rt_temporal_accumulate_cpu (librt_host.so, include/rt_host.h) return
 * the same bits.  Each device call is ONE stream-ordered kernel launch on hip_stream, allocates nothing, visits the host for nothing and
 * may be captured into a HIP graph at once.  One thread per output pixel, grid-stride; a pixel is written by one thread: no atomics.
 *
 * Planes are those of the denoise queries: a base pointer and a record stride in 4-byte WORDS, pixel i = r * cols + c at
 * base[i * stride + 0 .. width - 1] (width 3 for normal and position, 1 for object and valid), so rt_hit (13 words) and rt_surface (18
 * words) fields are passed where they lie: position = (const float *)hits + 3 and object = (const uint32_t *)hits + 2, stride 13;
 * normal = (const float *)surfaces + 14 and valid = (const uint32_t *)surfaces + 17, stride 18.  dot(a, b) is (a0*b0 + a1*b1) + a2*b2.
 * Every operation is a single f32 operation in the order written, none fused.
 *
 * rt_temporal_motion, for pixel i of the FULL previous frame (x0 = y0 = 0, x1 = width, y1 = height, y_step = 1; rows = height, cols =
 * width), with origin, cam_x, cam_y, cam_toward, half_width, half_height, height_f the camera basis every primary ray is shot with (of
 * prev_camera and prev_frame), P = position_i:
 *   1. v = P - origin
 *   2. z = dot(v, cam_toward)
 *   3. tt = dot(cam_x, cam_x)
 *   4. clip_x = dot(v, cam_x) / (z * tt)
 *   5. clip_y = dot(v, cam_y) / (z * tt)
 *   6. px = clip_x * height_f + half_width
 *   7. py = half_height - clip_y * height_f
 * the inverse of the primary ray through the image position (px, py).  motion_i = (px, py), 2 f32, in previous-frame pixel
 * coordinates; (NaN, NaN) (0x7fc00000) where valid is not NULL and valid_i == 0, or where z > 0 is false.  For a static scene position
 * is the current frame's position plane; for moving geometry it is the plane of where each point WAS in the previous frame, which
 * rt_previous_positions derives from the scene updates ("motion queries" above).  A caller may also write the motion plane itself.
 *
 * rt_temporal_accumulate, for output pixel p with current colour C = color[3 p + k], L = lum(C) = (0.2126f * C0 + 0.7152f * C1) +
 * 0.0722f * C2 and (px, py) = motion_p; history records are rt_temporal_pixel, read from history_in and written to history_out:
 *   1. p RESETS when current.valid is not NULL and valid_p == 0, or when any of px >= -1, px < (float)cols, py >= -1, py < (float)rows
 *      is false — float tests, made before any conversion to integer, false for a NaN, so 1e30 is refused, not wrapped.  A reset writes
 *      color = C (the raw words: a NaN keeps its payload), moment1 = L, moment2 = L * L, length = 1, and variance 0.
 *   2. otherwise fx = floor(px) (the truncation (float)(int64)px, less 1 where that is > px), wx = px - fx, likewise fy, wy; four taps
 *      q = (fy + j, fx + i), j = 0, 1 outer, i = 0, 1 inner, with b = (i ? wx : 1 - wx) * (j ? wy : 1 - wy).  A tap is skipped when
 *      b > 0 is false; when it lies outside the image; when previous.valid is not NULL and its word at q is 0; when history_in[q].length
 *      is 0; when object planes are given and previous.object_q != current.object_p; when normal planes are given and
 *      dot(n_p, n_q) >= normal_min is false; when position planes are given and, with d = P_p - P_q, dot(d, d) <= position_max *
 *      position_max is false (P_p is current.position — where the point was — and P_q previous.position at the tap).  An accepted tap
 *      adds: sum_k = sum_k + b * color_q[k], s1 = s1 + b * moment1_q, s2 = s2 + b * moment2_q, bsum = bsum + b (each product rounded
 *      before its add), and its length to the running minimum.  A NaN in an accepted tap's history propagates; nothing special-cases it.
 *   3. if bsum > 0 is false, p resets as in 1.
 *   4. otherwise H = sum / bsum (five divides), n = min(minimum length + 1, max_length) in integers, a = 1.0f / (float)n,
 *      alpha = a > alpha_min ? a : alpha_min, and out = H * (1 - alpha) + X * alpha for the three colours and the two moments with
 *      X = C_k, L, L * L;  length = n;  reserved words 0.
 *   5. variance_p (when d_variance is not NULL) = v > 0 ? v : +0 with v = moment2 - moment1 * moment1 of the record just written.
 * Consequences: integer (px, py) leaves one tap with b = 1, so H is that record exactly; with alpha_min = 0 and integer coordinates k
 * frames are the running mean written as the blend of 4; with max_length = 1 alpha is 1 and a finite history leaves the current frame.
 * A guide plane other than valid is either given in BOTH sets or NULL in both (its test is then off); valid may be NULL in either.
 * Checked before any device work, in this order, RT_ERR_INVALID_ARGUMENT unless said: rows * cols >= 2^32 (RT_ERR_UNSUPPORTED); rows ==
 * 0 or cols == 0 is RT_OK and launches nothing; a null guide set, params, color, motion, history_in or history_out; a stride smaller
 * than its plane's width; history_out == history_in; (device forms) a history array that is not 16-byte aligned; max_length < 1;
 * alpha_min outside [0, 1]; position_max >= 0 false; flags != 0; a plane given in one set and NULL in the other.  rt_temporal_motion: a
 * null camera or frame; a frame that is not the full frame; width * height >= 2^32 (RT_ERR_UNSUPPORTED); an empty frame is RT_OK; a null
 * position or motion; a stride smaller than its plane's width.
 * The variance-guided A-Trous that reads the variance plane, and the spatial variance estimate for short histories, are the
 * "variance-guided filter queries" below (rt_svgf_atrous, rt_svgf_variance).
 * Clamping the history to the neighbourhood's colour box is rt_temporal_accumulate_bounded of the "history rectification queries" below.
 * Not covered (moving geometry is: "motion queries" above): tiles and banded frames; rt_multi_* forms. */

typedef struct rt_temporal_pixel {
    float color[3];           /* the accumulated colour */
    float moment1;            /* ... luminance */
    float moment2;            /* ... squared luminance */
    uint32_t length;          /* frames accumulated, 1 .. max_length; 0: no history here (an array of zero bytes is an empty history) */
    uint32_t reserved[2];     /* written 0 */
} rt_temporal_pixel;         /* 32 bytes: a tap's history is two 16-byte loads */

typedef struct rt_temporal_guides {
    const float *normal;      /* 3 f32 per pixel, or NULL */
    const float *position;    /* 3 f32 per pixel, or NULL */
    const uint32_t *object;   /* 1 word per pixel, or NULL */
    const uint32_t *valid;    /* 1 word per pixel, 0: current — the pixel resets, previous — the pixel is no tap; or NULL */
    uint32_t normal_stride;   /* record strides in 4-byte words: >= 3 ... */
    uint32_t position_stride;
    uint32_t object_stride;   /* ... >= 1 */
    uint32_t valid_stride;    /* the stride of a NULL plane is not looked at */
} rt_temporal_guides;        /* 48 bytes */

typedef struct rt_temporal_params {
    float normal_min;         /* a tap passes when dot(n_p, n_q) >= normal_min */
    float position_max;       /* ... and |P_p - P_q| <= position_max; >= 0, +inf: every distance passes */
    float alpha_min;          /* the least weight of the current frame, in [0, 1]; 0: the running mean up to max_length */
    uint32_t max_length;      /* >= 1 */
    uint32_t flags;           /* reserved: 0 */
} rt_temporal_params;        /* 20 bytes */

/* d_position (and d_valid, or NULL): planes of prev_frame->width * height pixels; d_motion: 2 f32 per pixel, compact; one kernel launch */
int rt_temporal_motion(const float *d_position, uint32_t position_stride, const uint32_t *d_valid, uint32_t valid_stride,
                       const rt_camera *prev_camera, const rt_frame *prev_frame, float *d_motion, void *hip_stream);
/* d_color: rows * cols * 3 f32, d_motion: rows * cols * 2 f32, d_history_in / d_history_out: rows * cols records, two different arrays a
 * caller ping-pongs, 16-byte aligned; d_variance: rows * cols f32, or NULL; one kernel launch.  Nothing but d_history_out and d_variance
 * is written. */
int rt_temporal_accumulate(const float *d_color, const float *d_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                           const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *d_history_in,
                           rt_temporal_pixel *d_history_out, float *d_variance, void *hip_stream);
/* The same kernels on HOST arrays (the pointers of the guide sets are host pointers too): allocate, upload every plane with its
 * stride, run, synchronise the device and download.  NOT the CPU definition — that is rt_temporal_*_cpu of librt_host.so. */
int rt_temporal_motion_host(const float *h_position, uint32_t position_stride, const uint32_t *h_valid, uint32_t valid_stride,
                            const rt_camera *prev_camera, const rt_frame *prev_frame, float *h_motion);
int rt_temporal_accumulate_host(const float *h_color, const float *h_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *h_history_in,
                                rt_temporal_pixel *h_history_out, float *h_variance);

/* ---- history rectification queries: colour-box clamp and filtered feedback --------------------------

 * What keeps a history honest when shading changes and geometry does not — a light or a material was updated, a highlight slides over a
 * surface: rt_temporal_accumulate keeps a tap on geometry alone, so the stale colour fades at 1 / length only.  The defence is variance
 * clipping: the box mean +- gamma * deviation of the CURRENT frame's neighbourhood (rt_temporal_bounds), and the reprojected history
 * pulled into it before the blend (rt_temporal_accumulate_bounded).  rt_temporal_feedback writes a filtered colour back into the records,
 * which makes the filter below spatiotemporal — Schied et al.'s feedback of level 0:
 *     rt_temporal_motion -> rt_temporal_bounds -> rt_temporal_accumulate_bounded -> rt_svgf_variance -> rt_svgf_atrous (level 0)
 *         -> rt_temporal_feedback -> rt_svgf_atrous (levels 1 ..) -> rt_post_process_device
 * The reference has no counterpart; the definition below is the contract.  It is written once (csrc/rt_rectify.h, on csrc/rt_temporal.h
 * for everything the bounded accumulate shares with rt_temporal_accumulate) and compiled into both libraries without contraction, so the
 * device forms (any launch geometry), the _host forms and rt_temporal_bounds_cpu / rt_temporal_accumulate_bounded_cpu /
 * rt_temporal_feedback_cpu (librt_host.so, include/rt_host.h) return the same bits.  Each device call is ONE stream-ordered kernel launch
 * on hip_stream, allocates nothing, visits the host for nothing and may be captured into a HIP graph at once.  Every output word is
 * written by one thread: no atomics.  Planes, strides and lum(C) are the temporal block's; vpos and rtdm::f_sqrt the filter block's.
 * Every operation is a single f32 operation in the order written, none fused.
 *
 * rt_temporal_bounds, for output pixel p = (r, c).  color is 3 f32 per pixel at a word stride >= 3, read as rt_svgf_atrous reads it; a
 * pixel's four channels are x_0..2 = its colour and x_3 = lum of it.  The sources are the pixels q = (r + dr, c + dc), dr = -radius ..
 * radius (outer), dc = -radius .. radius (inner), both ascending, always at step 1; radius is 1, 2 or 3.  A source COUNTS when it lies
 * inside the image, valid is NULL or valid_q != 0, and object is NULL or object_q == object_p.  Two passes, per channel:
 *   1. s = +0, k = 0, and for each counting source in tap order:  s = s + x_q;  k = k + 1
 *   2. mean = s / (float)k
 *   3. v = +0, and in the same tap order over the same sources:  d = x_q - mean;  v = v + d * d
 *   4. var = vpos(v / (float)k)
 *   5. sd = rtdm::f_sqrt(var)
 *   6. half = gamma * sd
 *   7. lo = mean - half,  hi = mean + half
 * A pixel that does not count itself (valid_p == 0) gets lo = -inf, hi = +inf in all four channels: its history resets anyway.  A NaN in
 * a counting source propagates into mean, lo and hi of that channel; a NaN bound compares false and therefore clamps nothing.  The box
 * is a plane of its own and not fused into the accumulate so that a caller may fill rt_temporal_box itself (a min/max box, say).
 * Checked before any device work, in this order, RT_ERR_INVALID_ARGUMENT unless said: rows * cols >= 2^32 (RT_ERR_UNSUPPORTED); rows == 0
 * or cols == 0 is RT_OK and launches nothing; a null params, color or box; a stride smaller than its plane's width; radius outside 1 .. 3;
 * gamma >= 0 and finite false; flags != 0; (device form) a box array that is not 16-byte aligned.
 *
 * rt_temporal_accumulate_bounded: rt_temporal_accumulate with box_p = d_box[p] between its step 4's H = sum / bsum and the blend.  Steps 1
 * to 3 — the reset, the four taps, the sums — and n = min(minimum length + 1, max_length) are unchanged.  Then, for a p that did not reset:
 *   a. for k = 0 .. 2:  H'_k = H_k < lo_k ? lo_k : (H_k > hi_k ? hi_k : H_k)      (a NaN passes)
 *   b. the first moment likewise into [lo_3, hi_3]:  M1' = clamp(M1);  only where that changed M1:  M2' = M2 + (M1' * M1' - M1 * M1),
 *      so the history's variance is kept while its mean is shifted; otherwise M2 keeps its bits
 *   c. if any of the four was changed and clamped_length != 0:  n = min(n, clamped_length), before alpha = 1 / n is formed — a pixel whose
 *      history was contradicted answers at 1 / clamped_length instead of 1 / max_length
 * and the blend, the record, the variance plane and the reset are rt_temporal_accumulate's on H', M1', M2' and n.  d_clamped_p (when not
 * NULL) is the number of channels changed, 0 .. 4; 0 on a reset.  Consequence: with every box at (-inf, +inf) the records and the variance
 * are rt_temporal_accumulate's bit for bit, and d_clamped is 0.  Checked: everything rt_temporal_accumulate checks, in its order; then,
 * for an image that is not empty: a null box; (device form) a box array that is not 16-byte aligned; clamped_length > max_length.
 *
 * rt_temporal_feedback, in place on `history`: where valid is NULL or valid_p != 0, and history[p].length != 0, the record's three colour
 * words become the raw words of color_p (3 f32 at a word stride >= 3: a NaN keeps its payload); moments, length and reserved words keep
 * their bits, and every other record is untouched.  Checked, in this order: rows * cols >= 2^32 (RT_ERR_UNSUPPORTED); an empty image is
 * RT_OK; a null color or history; a stride smaller than its plane's width; (device form) a history array that is not 16-byte aligned.
 * RT_AMD_DIAG_RECTIFY_MAX_GROUPS (rt_set_option): a test hook, the three kernels launch at most this many workgroups and take the rest
 * of the image grid-stride; same bits.
 * Not covered: banded frames and rt_multi_* forms; a min/max box (a caller may write the box plane itself); the previous normal of
 * rotating surfaces. */

typedef struct rt_temporal_box {
    float lo[4];              /* k = 0 .. 2 colour, 3 luminance */
    float hi[4];
} rt_temporal_box;           /* 32 bytes: two 16-byte words */

typedef struct rt_bounds_params {
    float gamma;              /* the box is mean +- gamma * deviation; >= 0, finite */
    uint32_t radius;          /* 1, 2 or 3: a window of (2 radius + 1)^2 */
    uint32_t flags;           /* reserved: 0 */
} rt_bounds_params;          /* 12 bytes */

/* d_color: rows * cols pixels of 3 f32 at color_stride words; d_object, d_valid: one word per pixel at their strides, or NULL; d_box:
 * rows * cols boxes, 16-byte aligned; one kernel launch.  Nothing but d_box is written. */
int rt_temporal_bounds(const float *d_color, uint32_t color_stride, const uint32_t *d_object, uint32_t object_stride,
                       const uint32_t *d_valid, uint32_t valid_stride, const rt_bounds_params *params,
                       uint32_t rows, uint32_t cols, rt_temporal_box *d_box, void *hip_stream);
/* every argument of rt_temporal_accumulate, then d_box: rows * cols boxes, 16-byte aligned; clamped_length: 0 .. max_length, 0: the
 * length is not cut; d_clamped: rows * cols words, or NULL; one kernel launch */
int rt_temporal_accumulate_bounded(const float *d_color, const float *d_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                   const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *d_history_in,
                                   rt_temporal_pixel *d_history_out, float *d_variance, const rt_temporal_box *d_box,
                                   uint32_t clamped_length, uint32_t *d_clamped, void *hip_stream);
/* d_history: rows * cols records, 16-byte aligned, changed in place; one kernel launch */
int rt_temporal_feedback(const float *d_color, uint32_t color_stride, const uint32_t *d_valid, uint32_t valid_stride,
                         uint32_t rows, uint32_t cols, rt_temporal_pixel *d_history, void *hip_stream);
/* The same kernels on HOST arrays: allocate, upload every plane with its stride, run, synchronise the device and download.  NOT the CPU
 * definition — that is rt_temporal_bounds_cpu / rt_temporal_accumulate_bounded_cpu / rt_temporal_feedback_cpu of librt_host.so. */
int rt_temporal_bounds_host(const float *h_color, uint32_t color_stride, const uint32_t *h_object, uint32_t object_stride,
                            const uint32_t *h_valid, uint32_t valid_stride, const rt_bounds_params *params,
                            uint32_t rows, uint32_t cols, rt_temporal_box *h_box);
int rt_temporal_accumulate_bounded_host(const float *h_color, const float *h_motion, const rt_temporal_guides *current, const rt_temporal_guides *previous,
                                        const rt_temporal_params *params, uint32_t rows, uint32_t cols, const rt_temporal_pixel *h_history_in,
                                        rt_temporal_pixel *h_history_out, float *h_variance, const rt_temporal_box *h_box,
                                        uint32_t clamped_length, uint32_t *h_clamped);
int rt_temporal_feedback_host(const float *h_color, uint32_t color_stride, const uint32_t *h_valid, uint32_t valid_stride,
                              uint32_t rows, uint32_t cols, rt_temporal_pixel *h_history);

/* ---- variance-guided filter queries: the spatial half of SVGF -------------------------------------

 * What consumes the temporal block: a per-pixel luminance variance that is usable at every history length (rt_svgf_variance), and an
 * edge-avoiding A-Trous filter whose luminance weight is scaled by that variance and which filters the variance along with the colour
 * (rt_svgf_atrous) — the spatial half of Schied et al., "Spatiotemporal Variance-Guided Filtering" (HPG 2017):
 *     ... rt_temporal_motion -> rt_temporal_accumulate -> rt_svgf_variance -> rt_svgf_atrous -> rt_post_process_device
 * The reference has no counterpart; the definition below is the contract.  It is written once (csrc/rt_svgf.h, on pieces of
 * csrc/rt_denoise.h and csrc/rt_temporal.h where the operation is the same) and compiled into both libraries without contraction, so
 * the device forms (every kernel form, any launch geometry), the _host forms and rt_svgf_variance_cpu / rt_svgf_atrous_cpu (librt_host.so,
 * include/rt_host.h) return the same bits.  Every device call is stream-ordered and asynchronous on hip_stream, allocates nothing,
 * visits the host for nothing and may be captured into a HIP graph at once.  Every output word is written by one thread, which walks
 * its own taps in the order written here: no atomics, nothing depends on the launch.
 *
 * Planes are those of the two blocks above: a base pointer and a record stride in 4-byte WORDS, pixel i = r * cols + c; the guides are
 * rt_denoise_guides as they are.  Every operation is a single f32 operation in the order written, none fused.
 *   e(x)     x > 100 ? +0 : (float)rtdm::exp_mid(-(double)x)       as in step 3 of the denoise queries
 *   lum(C)   (0.2126f * C0 + 0.7152f * C1) + 0.0722f * C2          as in the temporal queries
 *   dist2    as in the denoise queries
 *   vpos(v)  v >= 0 ? v : +0      a negative or NaN variance reads as +0: THE rule wherever a variance is read
 *
 * rt_svgf_variance, for pixel p = (r, c) with record R_p of `history` (the records rt_temporal_accumulate just wrote):
 *   1. +0 when valid is not NULL and valid_p == 0, or when R_p.length == 0
 *   2. when R_p.length >= min_length:  v = moment2 - moment1 * moment1, written as v > 0 ? v : +0 — the bits rt_temporal_accumulate
 *      wrote to its variance plane
 *   3. otherwise s1 = s2 = wsum = +0, and for dr = -3 .. 3 (outer), dc = -3 .. 3 (inner), both ascending, always at step 1:
 *        q = (r + dr, c + dc);  skipped when outside the image, when valid is not NULL and valid_q == 0, or when R_q.length == 0
 *        x = +0;   if normal:  x = x + dist2(n_p, n_q) / sn2;   if position:  x = x + dist2(P_p, P_q) / sp2     (sn2, sp2: the squared sigmas)
 *        skipped unless x >= 0
 *        w = e(x);   s1 = s1 + moment1_q * w;   s2 = s2 + moment2_q * w;   wsum = wsum + w
 *      then, if wsum > 0:  a1 = s1 / wsum;  a2 = s2 / wsum;  v = a2 - a1 * a1;  v = v > 0 ? v : +0;  written:
 *      v * ((float)min_length / (float)R_p.length) — a short history's estimate is inflated, as in the paper;  otherwise +0.
 * A reset pixel (length 1, temporal variance +0) so gets the variance of its neighbourhood's first moments instead of "converged".
 * Consequences: with min_length = 1 the output is the temporal variance plane bit for bit; a pixel with length >= min_length does not
 * look at the guides.
 *
 * rt_svgf_atrous: d_color is 3 f32 per pixel at a word stride >= 3 (the colour inside the history records, stride 8, goes in where it
 * lies), d_variance one compact f32 per pixel, d_out a compact colour plane, d_variance_out a compact variance plane or NULL.  The
 * variance must be of the colour the filter SEES: a caller who demodulates passes the variance of the demodulated colour.
 * One level l (0 <= l <= 5), step s = 1 << l, input colour `in`, input variance `vin`, for output pixel p = (r, c):
 *   1. the colour seen at q:  C_q = in at q, divided by (albedo_q + 1e-3f) on a demodulating level exactly as in the denoise queries;
 *      l_q = lum(C_q);   V_q = vpos(vin_q)
 *   2. an invalid p (valid is not NULL and valid_p == 0) passes through: the colour's raw words and the variance's raw word
 *   3. the variance at p, prefiltered, always at step 1:  gs = ks = +0;  for dr = -1 .. 1 (outer), dc = -1 .. 1 (inner), each tap inside
 *      the image and valid, k = hk[dr + 1] * hk[dc + 1] with hk = {1/4, 1/2, 1/4}:   gs = gs + k * V_q;   ks = ks + k
 *      g = ks > 0 ? gs / ks : +0;    sl = sigma_luminance * (rtdm::f_sqrt(g) + 1e-6f)
 *   4. sum_k = vsum = wsum = +0, and dr, dc = -2 .. 2 at step s as in the denoise queries, with the same skip rules:
 *        d = |l_p - l_q|  (the sign bit cleared);   x = d / sl;   the normal and position terms added exactly as in the denoise queries
 *        skipped unless x >= 0
 *        w = h[dr + 2] * h[dc + 2] * e(x)
 *        sum_k = sum_k + C_q[k] * w;    vsum = vsum + V_q * (w * w);    wsum = wsum + w
 *   5. if wsum > 0:  out = sum_k / wsum, remodulated on a remodulating level;  variance_out = vsum / (wsum * wsum);
 *      otherwise p passes through as in 2.
 * sigma_luminance does not change with the level.  A call runs levels first_level .. first_level + n_levels - 1; they alternate between
 * d_temp and the outputs so that the LAST level writes d_out and d_variance_out; the inputs are only read.  flags are the
 * RT_DENOISE_DEMODULATE_* bits with the meaning they have in rt_denoise_atrous.  d_temp is opaque scratch of rt_svgf_temp_bytes bytes
 * (0 for one level).  Consequences: one call of n levels equals n calls of one level that chain (colour, variance), level j of them
 * with first_level + j, DEMODULATE_IN on the first only, DEMODULATE_OUT on the last only; for colours that are finite or NaN,
 * sigma_luminance = +inf gives the colour bits of rt_denoise_atrous with sigma_color = +inf on the same guides and flags.
 *
 * Checked before any device work, all RT_ERR_INVALID_ARGUMENT with a message that names the argument, in this order: a null guides or
 * params; rows * cols >= 2^32; (atrous) n_levels < 1 or first_level + n_levels > 6; a sigma that is not > 0 (NaN included; +inf is
 * legal); (variance) min_length < 1; unknown flag bits; a demodulation flag without an albedo plane; a stride smaller than its plane's
 * width; then rows == 0 or cols == 0 is RT_OK and launches nothing; a null required pointer (history, color, variance, out, the
 * variance call's variance_out; d_temp with n_levels >= 2); an output or the scratch equal to an input, to each other or to the scratch;
 * (device forms) a history array that is not 16-byte aligned.
 * Writing a filtered level back into the history records (SVGF's feedback of level 0) is rt_temporal_feedback, and clamping the history to
 * the neighbourhood's colour box rt_temporal_bounds / rt_temporal_accumulate_bounded, of the "history rectification queries" above.
 * Not covered: SVGF's depth-gradient and dot^128 normal weights — this block keeps the project's own normal and position terms; banded
 * frames and rt_multi_* forms. */

typedef struct rt_svgf_variance_params {
    float sigma_normal;
    float sigma_position;     /* each > 0, +inf: the term is off */
    uint32_t min_length;      /* >= 1: histories shorter than this take the spatial estimate */
    uint32_t flags;           /* reserved: 0 */
} rt_svgf_variance_params;   /* 16 bytes */

typedef struct rt_svgf_atrous_params {
    float sigma_luminance;    /* the same at every level: scaled per pixel by the square root of the prefiltered variance */
    float sigma_normal;
    float sigma_position;     /* each > 0, +inf: the term is off */
    uint32_t first_level;
    uint32_t n_levels;        /* first_level + n_levels <= RT_DENOISE_MAX_LEVELS */
    uint32_t flags;           /* RT_DENOISE_DEMODULATE_* */
} rt_svgf_atrous_params;     /* 24 bytes */

/* d_history: rows * cols records, 16-byte aligned; guides->albedo is not looked at; d_variance_out: rows * cols f32; one kernel launch */
int rt_svgf_variance(const rt_temporal_pixel *d_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                     uint32_t cols, float *d_variance_out, void *hip_stream);
/* what d_temp of rt_svgf_atrous must hold for a call of n_levels levels: 0 for one level, else 16 bytes per pixel (colour and variance
 * interleaved), and 4 more per pixel from three levels on */
size_t rt_svgf_temp_bytes(uint32_t rows, uint32_t cols, uint32_t n_levels);
/* one kernel launch per level; nothing but d_out, d_variance_out and d_temp is written */
int rt_svgf_atrous(const float *d_color, uint32_t color_stride, const float *d_variance, const rt_denoise_guides *guides,
                   const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *d_out, float *d_variance_out, void *d_temp,
                   void *hip_stream);
/* The same kernels on HOST arrays (the pointers of `guides` are host pointers too): allocate, upload every plane with its stride, run,
 * synchronise the device and download.  No h_temp: the round trip makes its own.  NOT the CPU definition — that is rt_svgf_*_cpu of
 * librt_host.so. */
int rt_svgf_variance_host(const rt_temporal_pixel *h_history, const rt_denoise_guides *guides, const rt_svgf_variance_params *params, uint32_t rows,
                          uint32_t cols, float *h_variance_out);
int rt_svgf_atrous_host(const float *h_color, uint32_t color_stride, const float *h_variance, const rt_denoise_guides *guides,
                        const rt_svgf_atrous_params *params, uint32_t rows, uint32_t cols, float *h_out, float *h_variance_out);

/* ---- guided upsampling queries: low-resolution radiance onto full-size guides ------------------------

 * What makes a frame cheaper everywhere instead of where it is easy: the radiance — the expensive part — rendered at 1/s of the
 * resolution each way, the guide planes (rt_probe_surfaces on the primary hits: position, shading normal, albedo, object, valid) at
 * full resolution, and the radiance carried up onto them by a joint bilateral upsample (Kopf et al., "Joint Bilateral Upsampling",
 * SIGGRAPH 2007).  With the albedo divided out below and multiplied back above, texture detail returns at full resolution; the object
 * test and the normal and position terms keep geometric edges sharp.
 *     rt_probe_surfaces (low) -> radiance (low) -> rt_probe_surfaces (full) -> rt_upsample_guided -> rt_post_process_device
 * The low image is taken at the CENTRES of the s x s blocks of output pixels (step 2).  rt_camera_rays shoots through a pixel's integer
 * coordinate, so the low frame's own rays look where output pixel j s looks, (s - 1) / 2 output pixels off: take the low rays from
 * rt_camera_rays_offset on the low frame with the offset (s - 1) / (2 s) both ways, and trace and probe those.
 * The reference has no counterpart; the definition below is the contract.  It is written once (csrc/rt_upsample.h, on the guide readers,
 * the weight terms and e(x) of csrc/rt_atrous.h) and compiled into both libraries without contraction, so the device form (either
 * kernel form, any launch geometry), the _host form and rt_upsample_guided_cpu (librt_host.so, include/rt_host.h) return the same bits.
 * The device call is ONE stream-ordered kernel launch on hip_stream, allocates nothing, visits the host for nothing and may be captured
 * into a HIP graph at once.  Every output word is written by one thread: no atomics, nothing depends on the launch.
 *
 * Planes are those of the denoise queries: a base pointer and a record stride in 4-byte WORDS, pixel i = r * cols + c.  rows and cols
 * are the OUTPUT's; the low-resolution image has rows_lo = ceil(rows / s) rows and cols_lo = ceil(cols / s) columns, s = scale, derived
 * and not passed.  color_lo: 3 f32 per low pixel at color_stride words (the colour inside rt_temporal_pixel records, stride 8, goes in
 * where it lies).  `low` and `full` are rt_denoise_guides of the two resolutions; object_lo / object_full one word per pixel at their
 * strides, or NULL.  out: 3 f32 per output pixel, compact.  A guide term is ON where both guide sets carry its plane; the object test
 * is on where both object planes are given.  Every operation is a single f32 operation in the order written, none fused; e(x) and dist2
 * are the denoise queries'.  For output pixel p = (r, c), with R = radius:
 *   1. nearest: N = (r / s, c / s) in integer division, a pixel of the low image.  If full->valid is not NULL and valid_p == 0, out_p is
 *      the raw words of color_lo at N (a NaN keeps its payload), and nothing else is looked at.
 *   2. the position in the low grid, in integers:  a = 2 r + 1 - s;   b_y = floor(a / 2 s)  (a floor: a is negative on the first rows);
 *      n_y = a - 2 s * b_y  (0 .. 2 s - 1);   f_y = (float)n_y / (float)(2 s);   b_x, f_x the same from c.  The centre of output pixel r
 *      lies at (2 r + 1 - s) / 2 s low pixels from the centre of low pixel 0.
 *   3. sum_k = wsum = +0, and for dr = -(R - 1) .. R (outer), dc = -(R - 1) .. R (inner), both ascending, the source q = (b_y + dr, b_x + dc):
 *        t_y = 1 - fabsf((float)dr - f_y) / (float)R;    t_x = 1 - fabsf((float)dc - f_x) / (float)R
 *        skipped when t_y <= 0 or t_x <= 0; when q is outside the low image; when low->valid is not NULL and valid_q == 0
 *        C_q = color_lo at q, divided by (albedo_q + 1e-3f) of the LOW albedo with RT_DENOISE_DEMODULATE_IN, channel by channel
 *        skipped unless all three channels of C_q are finite (C - C == 0): one inf or NaN sample does not become a block of s x s
 *        skipped when the object test is on and object_q != object_p
 *        x = +0;   if normal:  x = x + dist2(n_p, n_q) / sn2;   if position:  x = x + dist2(P_p, P_q) / sp2     (sn2, sp2: the squared sigmas;
 *        n_p, P_p of `full`, n_q, P_q of `low`);   skipped unless x >= 0
 *        w = (t_y * t_x) * e(x);    sum_k = sum_k + C_q[k] * w;    wsum = wsum + w
 *   4. if wsum > 0:  out_k = sum_k / wsum, multiplied by (albedo_p + 1e-3f) of the FULL albedo with RT_DENOISE_DEMODULATE_OUT;
 *      otherwise out_p is the raw words of color_lo at N, as in 1.
 * Consequences: with radius 1, both sigmas +inf and no object planes, valid everywhere, the result is the bilinear interpolation of the
 * low image whose pixel centres coincide with step 2's positions, renormalised at the border; a constant low image whose value is a
 * power of two returns itself; where the object test is on no colour crosses an object's edge.
 *
 * Checked before any device work, all RT_ERR_INVALID_ARGUMENT with a message that names the argument, in this order: a null params,
 * low or full; rows * cols >= 2^32; scale outside 2 .. 4; radius outside 1 .. 2; a sigma that is not > 0 (NaN included; +inf is legal:
 * the term is off); unknown flag bits; RT_DENOISE_DEMODULATE_IN without low->albedo, RT_DENOISE_DEMODULATE_OUT without full->albedo;
 * a stride smaller than its plane's width (the guides of low, of full, color_stride < 3, an object stride < 1 of a plane that is
 * given); then rows == 0 or cols == 0 is RT_OK and launches nothing; a null color_lo or out; out == color_lo.
 * RT_AMD_UPSAMPLE_FORM (rt_set_option): 0 the plain kernel, every source read from global memory; 1 the tiled kernel, a workgroup's
 * low-resolution window staged in LDS once; same bits (DESIGN.md 3.28 says which is the default and why).  RT_AMD_DIAG_UPSAMPLE_MAX_GROUPS:
 * a test hook, the kernel launches at most this many workgroups and takes the rest of the image grid-stride; same bits.
 * Not covered: banded frames and rt_multi_* forms; fractional scales and scales beyond 4; the variance plane and history records (a
 * caller upsamples colour); a jitter of the low-resolution grid from frame to frame. */

typedef struct rt_upsample_params {
    float sigma_normal;
    float sigma_position;     /* each > 0, +inf: the term is off */
    uint32_t scale;           /* s: 2, 3 or 4 output pixels per low pixel, each way */
    uint32_t radius;          /* R: 1 or 2, a window of (2 R)^2 low pixels; 1 is the bilinear footprint */
    uint32_t flags;           /* RT_DENOISE_DEMODULATE_* */
} rt_upsample_params;        /* 20 bytes */

/* d_color_lo: ceil(rows / s) * ceil(cols / s) pixels of 3 f32 at color_stride words; low / d_object_lo: planes of that many pixels;
 * full / d_object_full: planes of rows * cols pixels; d_out: rows * cols * 3 f32; one kernel launch.  Nothing but d_out is written. */
int rt_upsample_guided(const float *d_color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *d_object_lo,
                       uint32_t object_lo_stride, const rt_denoise_guides *full, const uint32_t *d_object_full, uint32_t object_full_stride,
                       const rt_upsample_params *params, uint32_t rows, uint32_t cols, float *d_out, void *hip_stream);
/* The same kernel on HOST arrays (the pointers of the guide sets are host pointers too): allocate, upload every plane with its stride,
 * run, synchronise the device and download.  NOT the CPU definition — that is rt_upsample_guided_cpu of librt_host.so. */
int rt_upsample_guided_host(const float *h_color_lo, uint32_t color_stride, const rt_denoise_guides *low, const uint32_t *h_object_lo,
                            uint32_t object_lo_stride, const rt_denoise_guides *full, const uint32_t *h_object_full, uint32_t object_full_stride,
                            const rt_upsample_params *params, uint32_t rows, uint32_t cols, float *h_out);

/* ---- diagnostics ------------------------------------------------------------ */

/* Which kernel renders the Whitted pass (process-wide; same results bit for bit):
 *   18 (default)  the persistent wavefront kernel (csrc/rt_pwf.hip): one kernel whose workgroups keep queues of single-cast
 *                 work items (a ray_trace activation's own cast, one cast of get_refract, one shadow cast of get_shade)
 *                 and fold the results bottom-up at the end; a frame that does not fit its arenas is rendered by the
 *                 per-pixel kernel (2) within the same call
 *   2             the per-pixel kernel (csrc/rt_kernels.hip): one work-item per primary ray, a wave = an 8x8 tile, the
 *                 recursion unrolled into a per-lane state machine; triangle records fetched with wave-uniform scalar loads
 *   3, 19         as 2 / 18 with the per-pixel kernel's triangle records staged in LDS once per workgroup (the north_star's
 *                 wording; slower than the scalar fetches: DESIGN.md, profiles/)
 * or the value of the RT_AMD_VARIANT environment variable at load.  Anything else is RT_ERR_INVALID_ARGUMENT. */
/* Process-wide switches: settings of the launch plumbing and test hooks, none of which changes a result.  Each is an integer
 * named like the environment variable that seeds it — RT_AMD_DIST_PIPELINE, RT_AMD_DIST_WS_MB, RT_AMD_RNG_LOOKAHEAD,
 * RT_AMD_DIST_BY_COST, RT_AMD_DIST_OWN_FIRST, RT_AMD_DIST_PREP_FIRST, RT_AMD_DIST_SPLIT, RT_AMD_DIAG_WS_REFUSE,
 * RT_AMD_MULTI_FORCE_STAGE, RT_AMD_BFS_WALK_TRIANGLES (read by rt_scene_create), RT_AMD_WF_SHARE, RT_AMD_DIAG_BFS_CAP,
 * RT_AMD_DIAG_DIST_BAND_RAYS, RT_AMD_QUERY_WAVE_UNIFORM, RT_AMD_DIAG_HIT_BAND_RECORDS, RT_AMD_FILM_SPLAT_FORM, RT_AMD_DIAG_FILM_MAX_GROUPS,
 * RT_AMD_DENOISE_FORM, RT_AMD_DIAG_DENOISE_MAX_GROUPS, RT_AMD_DIAG_TEMPORAL_MAX_GROUPS, RT_AMD_SVGF_FORM, RT_AMD_DIAG_SVGF_MAX_GROUPS, RT_AMD_DIAG_MOTION_MAX_GROUPS, RT_AMD_DIAG_RECTIFY_MAX_GROUPS, RT_AMD_DIAG_ADAPTIVE_MAX_GROUPS, RT_AMD_UPSAMPLE_FORM, RT_AMD_DIAG_UPSAMPLE_MAX_GROUPS, RT_AMD_BLOOM_FORM, RT_AMD_DIAG_BLOOM_MAX_GROUPS (INTEGRATION.md says what each does); any other name is RT_ERR_INVALID_ARGUMENT.  The environment is read ONCE per process, at the first use;
 * after that only this call changes a switch: value = decimal integer, NULL or "" = unset (the library's own choice).  Render
 * calls read the switches without locks: set them between calls, not during one. */
int rt_set_option(const char *name, const char *value);
int rt_set_variant(int variant);
int rt_get_variant(void);

/* Persistent-wavefront path (variant bit 4): size of its arenas, in ray_trace activations per tile pixel (default 6,
 * RT_AMD_WF_NODES_PER_PIXEL; the reference scene needs 3.4 at depth 8; about 200 B of device memory each, rounded up
 * to a power of two per workgroup).  A frame that needs more is detected on the device and rendered by the per-pixel
 * kernel within the same call, so the budget changes speed and memory only, never results.  Arenas are never smaller
 * than 1.5 MB per workgroup unless the budget is below 4. */
int rt_set_wavefront_budget(unsigned nodes_per_pixel);

/* rt_render_distributed has two organisations with bit-identical results (samples, flags, RNG states, cast counts):
 *   1 (default)  three kernels per batch of epochs — the scatter chain with all random draws, every get_shade it
 *                asked for, the unwind + filter + accumulation — over a per-stream workspace (852 B per sample at depth 8,
 *                at most RT_AMD_DIST_WS_MB MiB, default 32768 for a call of several batches — which uses two workspaces in turn,
 *                batch k's get_shade and unwind kernels running beside batch k+1's chain kernel on streams the rt_rng owns, all of
 *                them behind the caller's stream again when the call returns (RT_AMD_DIST_PIPELINE=0: one workspace, in line) — and
 *                16384 for one of a single batch; a batch is as many epochs as fit, 16 at most, and fewer if the device cannot
 *                provide the memory — down to organisation 0 when not even one epoch fits; a workspace that holds at least half
 *                the batch wanted is kept rather than replaced);
 *   2            round 2's queued chain kernel: measured slower than 1 twice and removed in round 3 — the value now selects 1;
 *   0            one kernel, a lane stays on its pixel through chain, shades and unwind (no workspace).
 * -1 restores the default / the RT_AMD_DIST_SPLIT environment variable. */
int rt_set_distributed_split(int on);

/* Timing of the dominant (render) kernel alone: while enabled, each rt_render_whitted call records a HIP
 * event pair on its stream right around that kernel (a call may also launch a small probe kernel);
 * rt_profile_read synchronises the device, returns the summed elapsed milliseconds and the number of
 * launches since the last read, and resets. */
int rt_profile_enable(int on);
int rt_profile_read(double *kernel_ms_sum, unsigned *n_launches);
/* The same for the depth-of-field pass: while profiling is enabled, rt_render_distributed (the chain / shade / unwind organisation)
 * brackets every kernel launch with an event pair on the stream the launch is put on; this synchronises the device and returns, per
 * kernel — [0] the generators' look-ahead (rng_scan + rng_prepare), [1] dist_chain_kernel, [2] the shade kernel, [3] dist_unwind_kernel —
 * the summed milliseconds and the launches since the last read, and resets.  Kernels of a pipelined call overlap: these are each
 * kernel's own durations under that overlap (what a kernel trace shows), not shares of the call's wall time. */
int rt_profile_read_distributed(double ms_sum[4], unsigned n_launches[4]);

/* The deterministic f32 math the path computes with (csrc/rt_detmath.h),
 * evaluated element-wise on the host or on the device, so tests can prove the
 * two return identical bits.  op is an rt_math_op; y is ignored by unary ops.
 * The *_HI/_LO ops return the two 32-bit halves of a binary64 result
 * reinterpreted as f32 bit patterns (for checking f64 sqrt/div rounding). */
typedef enum rt_math_op {
    RT_MATH_SIN = 0, RT_MATH_COS = 1, RT_MATH_TAN = 2, RT_MATH_ACOS = 3,
    RT_MATH_ATAN2 = 4,   /* atan2(x, y): x is the ordinate */
    RT_MATH_POW = 5,     /* pow(x, y) */
    RT_MATH_F32_DIV = 6, RT_MATH_F32_SQRT = 7,
    RT_MATH_F64_SQRT_HI = 8, RT_MATH_F64_SQRT_LO = 9,   /* sqrt((double)x * (double)y) */
    RT_MATH_F64_DIV_HI = 10, RT_MATH_F64_DIV_LO = 11,   /* (double)x / (double)y */
    RT_MATH_ROUND = 12,
    RT_MATH_SINCOS_SIN = 13, RT_MATH_SINCOS_COS = 14,   /* the two results of the fused sincosf the kernels call */
    RT_MATH_F32_AS_I32 = 15,  /* f32_as_i32(x), the i32 as an f32 bit pattern */
    RT_MATH_IS_NORMAL = 16,   /* is_normal(x): 0.0f or 1.0f */
    RT_MATH_INT_CLASS = 17    /* f32_int_class(x) as a float: 0 not an integer, 1 odd, 2 even */
} rt_math_op;
int rt_math_eval_host(int op, const float *x, const float *y, float *out, size_t n);
int rt_math_eval_device(int op, const float *h_x, const float *h_y, float *h_out, size_t n);

/* The binary64 primitives those f32 results rest on, and three binary64 intermediates, each returned as a whole double so that
 * tests compare all 64 bits of host and device.  op is an rt_math64_op; b is ignored by unary ops (and may be NULL).  Operands
 * outside an op's stated domain are the caller's mistake: nothing is checked. */
typedef enum rt_math64_op {
    RT_MATH64_DIV = 0,          /* a / b */
    RT_MATH64_SQRT = 1,         /* d_sqrt(a) */
    RT_MATH64_NARROW = 2,       /* (double)(float)a: the f64 -> f32 rounding */
    RT_MATH64_ROUND_I32 = 3,    /* (double)d_round_to_i32(a), |a| < 2^31 - 1 */
    RT_MATH64_FROM_I64 = 4,     /* (double)(int64_t)bits(a): a's bit pattern read as an i64 and converted */
    RT_MATH64_EXP_MID = 5,      /* exp_mid(a), |a| <= 200 */
    RT_MATH64_LOG_POS = 6,      /* log_pos(a), finite a > 0 */
    RT_MATH64_ATAN2_UPPER = 7   /* atan2_upper(a, b): a >= 0 the ordinate, not NaN, not both zero or both infinite */
} rt_math64_op;
int rt_math_eval64_host(int op, const double *a, const double *b, double *out, size_t n);
int rt_math_eval64_device(int op, const double *h_a, const double *h_b, double *h_out, size_t n);

/* The node array rt_scene_create builds over the triangles for the intersection loop (csrc/rt_device_scene.h: a pre-order
 * array of leaves — runs of consecutive triangles — and inner nodes with skip pointers), computed on the host without
 * touching a device: six words per node — first triangle, count (0: inner node), n_normals (0: plain leaf, always
 * visited; 0xffffffff: a normal cone), skip_to, the pair-wise dealing word (chunk | chunks << 8 | sub-jobs per pass << 16; 0:
 * never pair-wise), 0.  Writes at most cap_nodes nodes, always reports the count.  For tests of the builder's invariants. */
int rt_scene_describe_nodes(const rt_scene_desc *desc, uint32_t *out_words, uint32_t cap_nodes, uint32_t *n_nodes);

/* What the shortcuts that skip work of a certain outcome would be given for `desc`, computed on the host without touching a device by
 * the code rt_scene_create runs: per triangle the centre and the padded squared radius of its bounding sphere (tri4: bcx, bcy, bcz, bq;
 * bq = +inf: no rejection for this triangle), per sphere the squared distance above which a ray misses before the root is taken
 * (sphere1: q_miss; +inf: never), per light the cosines outside which a spot light's cone is decided without the arc cosine (light2:
 * cos_in, cos_out; +inf and -inf: never), and the squared origin distance up to which a ray uses the bounding-sphere rejections at all
 * (*filter_origin2).  Each array holds one entry per primitive of `desc`; any of the four outputs may be NULL.  For tests that aim at
 * those margins. */
int rt_scene_describe_filters(const rt_scene_desc *desc, float *tri4, float *sphere1, float *light2, float *filter_origin2);

/* The node records of a scene as they stand on the device, copied to host memory with a blocking copy: `which` 0 the pre-order
 * array (csrc/rt_device_scene.h DevSegment, 40 words per node), 1 the same records in level order (an inner node's first / skip_to
 * name its children there), 2 the 16-byte pieces of the breadth-first walk (per node in level order: first, count, n_normals, r2_hi;
 * then centre and child count; then the first plane direction or the cone; then two pieces per triangle).  Always reports the
 * number of 32-bit words in *n_words and copies only when cap_words holds them all.  The caller has synchronised every stream that
 * updates the scene.  For tests of rt_scene_update_vertices: what it leaves against what rt_scene_create builds. */
int rt_diag_scene_nodes(const rt_scene *scene, int which, uint32_t *h_words, size_t cap_words, size_t *n_words);

/* Which code a Whitted call on the persistent-wavefront path runs.  The kernel has eight instantiations, pwf_kernel<PACKED, BFS, RAYS>
 * (csrc/rt_pwf_kernel.h), and the launcher picks one per call: PACKED from the arenas' size (csrc/rt_pwf_common.h pa_ready_packed),
 * BFS for a scene walked breadth-first (RT_AMD_BFS_WALK_TRIANGLES at rt_scene_create) whose lists the stream's workspace holds, RAYS
 * for a ray batch.  rt_diag_pwf_plan reports, for `frame` rendered on `hip_stream` (rt_render_whitted; the camera does not matter),
 * what the launcher computes from the frame, the scene, the current rt_set_wavefront_budget and RT_AMD_WF_SHARE, with the stream's
 * workspace as it stands — it calls the launcher's own functions, allocates nothing, launches nothing and changes nothing.
 * rt_diag_pwf_plan_rays is the same for a batch of n_rays rays at max_depth (rt_trace_rays).  Workspaces only grow and are made by the
 * first call that needs them, so ask AFTER the call in question, the settings unchanged: the answer is then what that call launched.
 * out_words receives RT_DIAG_PWF_PLAN_WORDS words:
 *   RT_DIAG_PWF_PERSISTENT  1: the call launches the persistent kernel (the variant has it, the scene fits its items, the workspace
 *                           holds the arenas and, for BFS, the lists); 0: the per-pixel kernel renders the frame
 *   RT_DIAG_PWF_GROUPS      workgroups of the grid, one arena each
 *   RT_DIAG_PWF_UNITS       rows of the frame, or rays of the batch
 *   RT_DIAG_PWF_BAND_UNITS  ... of them per launch: below UNITS the call is several bands, one launch each
 *   RT_DIAG_PWF_RING_CAP, RT_DIAG_PWF_NODE_CAP   ring slots and nodes per arena
 *   RT_DIAG_PWF_PACKED, RT_DIAG_PWF_BFS, RT_DIAG_PWF_RAYS   the three template arguments, 0 or 1 each
 *   RT_DIAG_PWF_BUDGET      the nodes per pixel the plan was made for
 * For tests that must know which instantiation they ran. */
#define RT_DIAG_PWF_PERSISTENT 0
#define RT_DIAG_PWF_GROUPS 1
#define RT_DIAG_PWF_UNITS 2
#define RT_DIAG_PWF_BAND_UNITS 3
#define RT_DIAG_PWF_RING_CAP 4
#define RT_DIAG_PWF_NODE_CAP 5
#define RT_DIAG_PWF_PACKED 6
#define RT_DIAG_PWF_BFS 7
#define RT_DIAG_PWF_RAYS 8
#define RT_DIAG_PWF_BUDGET 9
#define RT_DIAG_PWF_PLAN_WORDS 10
int rt_diag_pwf_plan(const rt_scene *scene, const rt_frame *frame, void *hip_stream, uint32_t *out_words);
int rt_diag_pwf_plan_rays(const rt_scene *scene, size_t n_rays, int32_t max_depth, void *hip_stream, uint32_t *out_words);

/* How the last rt_render_whitted / rt_trace_rays call on `hip_stream` ended on the persistent-wavefront path: a frame the arenas cannot
 * finish raises an overflow flag and the trailing per-pixel launch renders it, with the same pixels and cast count, so results cannot
 * tell the two apart.  The flag lives in the block of counters the call's launch took, which stays as the kernel left it until the
 * next launch on that workspace; this copies it out behind the stream's work and waits for the copy (the kernel writes nothing for
 * it).  A call of several bands reuses one block, so what is reported is its LAST band.  Direct calls only, not graph replays.
 * out_words receives RT_DIAG_PWF_OUTCOME_WORDS words, all 0 when that call launched no persistent kernel:
 *   RT_DIAG_PWF_LAUNCHED    1: the call launched the persistent kernel
 *   RT_DIAG_PWF_OVERFLOW    1: the frame (band) was not finished within the arenas and the per-pixel kernel rendered it
 *   RT_DIAG_PWF_TILES_DONE  64-pixel tiles whose pixels the persistent kernel wrote
 *   RT_DIAG_PWF_GROUPS_DONE workgroups that left the kernel (all of them)
 *   RT_DIAG_PWF_CASTS_LO, RT_DIAG_PWF_CASTS_HI   the casts the persistent kernel counted (added to the caller's count only without overflow) */
#define RT_DIAG_PWF_LAUNCHED 0
#define RT_DIAG_PWF_OVERFLOW 1
#define RT_DIAG_PWF_TILES_DONE 2
#define RT_DIAG_PWF_GROUPS_DONE 3
#define RT_DIAG_PWF_CASTS_LO 4
#define RT_DIAG_PWF_CASTS_HI 5
#define RT_DIAG_PWF_OUTCOME_WORDS 6
int rt_diag_pwf_outcome(const rt_scene *scene, void *hip_stream, uint32_t *out_words);

#ifdef __cplusplus
}
#endif
#endif /* RT_AMD_H */
