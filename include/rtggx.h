/*
 * rtggx.h -- C ABI of librtggx, the MI355X (gfx950) implementation of the RayTracedGGX hot path.
 *
 * This is the drop-in boundary: each entry point replaces one method of the
 * reference's pass objects, minus the D3D12 handle parameters.  The reference-side binding a
 * maintainer would add is shown in INTEGRATION.md.  No C++ or torch types cross this boundary;
 * every function returns 0 on success or a negative code (text via rtggx_last_error()).
 * A context is used from one host thread and owns all device memory; host arrays passed to
 * rtggx_set_* are copied before the call returns.
 *
 *   reference interface (RayTracedGGX/...)                          entry point
 *   -------------------------------------------------------------   ---------------------------
 *   RayTracer::Init            Content/RayTracer.h:24-29, .cpp:66    rtggx_create + rtggx_set_mesh + rtggx_set_env
 *   Denoiser::Init             Content/Denoiser.h:15-17, .cpp:21     rtggx_create (render targets of both)
 *   createVB/createIB/createGroundMesh   RayTracer.cpp:393-511       rtggx_set_mesh
 *   DDS::Loader::CreateTextureFromFile   RayTracer.cpp:143-150       rtggx_set_env
 *   buildAccelerationStructures + BuildAccelerationStructures        rtggx_build_as
 *                              RayTracer.cpp:676-716, 158-233
 *   RayTracer::SetMetallic     RayTracer.cpp:244-248                 rtggx_set_metallic
 *   CBMaterial upload          RayTracer.cpp:129-140                 rtggx_set_material
 *   RayTracer::UpdateFrame     RayTracer.cpp:250-305 (constants)     rtggx_update_frame
 *   RayTracer::UpdateAccelerationStructure   RayTracer.cpp:326-341   rtggx_update_as
 *   RayTracer::TransformSH     RayTracer.cpp:307-310                 rtggx_transform_sh
 *   RayTracer::RenderVisibility RayTracer.cpp:343-365, 751-791       rtggx_render_visibility
 *   RayTracer::RayTrace        RayTracer.cpp:367-376, 793-810        rtggx_ray_trace
 *   Denoiser::Denoise          Denoiser.cpp:66-75                    rtggx_denoise
 *   Denoiser::ToneMap          Denoiser.cpp:77-103                   rtggx_tone_map
 *   GetRayTracingOutputs/GetGBuffers/GetDepth  RayTracer.cpp:378-391 rtggx_readback / rtggx_buffer_ptr
 *   WaitForGpu                 RayTracedGGX.cpp:672-682              rtggx_sync
 */
#ifndef RTGGX_H
#define RTGGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtggx_context rtggx_context;

enum { RTGGX_GROUND = 0, RTGGX_MODEL_OBJ = 1, RTGGX_NUM_MESH = 2 };   /* RayTracer::MeshIndex, RayTracer.h:13-19 */

/* Constant buffers of the reference, byte for byte.  4x4 matrices are
 * stored as the reference uploads them (XMStoreFloat4x4 of the transpose): logical row-vector
 * matrix M[i][j] = f[j*4+i].  3x4 blocks are XMStoreFloat3x4 images. */
typedef struct RtggxCBGlobal {            /* RayTracer.cpp:27-35  <->  RayTracing.hlsl:46-53 */
  float    WorldViewProjs[2][16];
  float    WorldViewProjsPrev[2][16];
  float    Worlds[2][12];
  float    WorldITs0[12];
  float    WorldIT1[11];
  uint32_t FrameIndex;
} RtggxCBGlobal;
typedef struct RtggxRayGenConstants {     /* RayTracer.cpp:20-25  <->  RayTracing.hlsl:55-60 */
  float ProjToWorld[16];
  float EyePt[4];
  float ProjBias[2];
  float pad[2];
} RtggxRayGenConstants;
typedef struct RtggxCBPerObject {         /* RayTracer.cpp:37-41  <->  VSVisibility.hlsl:17-21 */
  float WorldViewProj[16];
  float ProjBias[2];
  float pad[2];
} RtggxCBPerObject;
typedef struct RtggxCBMaterial {          /* RayTracer.cpp:43-47  <->  Material.hlsli:10-14 */
  float BaseColors[2][4];
  float RoughMetals[2][4];
} RtggxCBMaterial;
typedef struct RtggxFrameConstants {      /* 768 bytes */
  RtggxCBGlobal        global;
  RtggxRayGenConstants rayGen;
  RtggxCBPerObject     perObject[2];
  RtggxCBMaterial      material;          /* ignored by rtggx_update_frame: CBMaterial is persistent, see rtggx_set_material */
} RtggxFrameConstants;

/* Environment texel formats accepted by rtggx_set_env (DXGI numbering). */
enum { RTGGX_FORMAT_RGBA32F = 2, RTGGX_FORMAT_RGBA16F = 10, RTGGX_FORMAT_BC6H_UF16 = 95, RTGGX_FORMAT_BC6H_SF16 = 96 };

/* Buffers readable with rtggx_readback (one element per pixel unless noted). */
enum {
  RTGGX_BUF_VISIBILITY = 0,  /* uint32  ((instance<<24)|primitive)+1, 0 = empty   PSVisibility.hlsl:23 */
  RTGGX_BUF_DEPTH = 1,       /* uint32  D24 value in the low 24 bits */
  RTGGX_BUF_NORMAL = 2,      /* uint32  R10G10B10A2_UNORM */
  RTGGX_BUF_ROUGH_METAL = 3, /* uint16  R8G8_UNORM */
  RTGGX_BUF_VELOCITY = 4,    /* uint32  R16G16_FLOAT */
  RTGGX_BUF_RT_REFL = 5,     /* uint32  R11G11B10_FLOAT, RayTracingOut0 */
  RTGGX_BUF_RT_DIFF = 6,     /* uint32  R11G11B10_FLOAT, RayTracingOut1 */
  RTGGX_BUF_TSS0 = 7,        /* uint64  R16G16B16A16_FLOAT, TemporalSSOut0 */
  RTGGX_BUF_TSS1 = 8,        /* uint64  TemporalSSOut1 */
  RTGGX_BUF_FLT_RFL = 9,     /* uint64  FilteredOut (with no diffuse pass to read it -- both instances fully metallic -- it equals FilteredOut1
                                bit for bit and only that one is written: readback and buffer_ptr then return FilteredOut1) */
  RTGGX_BUF_FLT_DFF = 10,    /* uint64  FilteredOut1 */
  RTGGX_BUF_BACKBUFFER = 11, /* uint32  R8G8B8A8_UNORM */
  RTGGX_BUF_SH_COEFFS = 12,  /* 27 floats: 9 x float3 */
  RTGGX_BUF_BVH_NODES0 = 13, /* 64-byte nodes of mesh 0 (see DESIGN.md "BVH layout") */
  RTGGX_BUF_BVH_TRIS0 = 14,  /* 64-byte leaf triangles of mesh 0: v0,v1,v2 (9 floats), 3 pad, primitive id (word 12), 3 pad */
  RTGGX_BUF_BVH_NODES1 = 15,
  RTGGX_BUF_BVH_TRIS1 = 16,
  RTGGX_BUF_TLAS = 17,       /* 2 x 16 floats: world->object matrices (row-vector, row-major) */
  RTGGX_BUF_ENV = 18,        /* decoded RGBA16F environment, mip-major, 6 faces per mip */
  RTGGX_BUF_BVH4_NODES0 = 19, /* 128-byte 4-wide nodes of mesh 0, indexed like the binary nodes (the slots of binary nodes folded into another: zero): */
  RTGGX_BUF_BVH4_NODES1 = 20, /*   minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4] ref[4] pad[4]; ref: >=0 node, <0 ~leaf slot, 0x7FFFFFFF none */
  RTGGX_BUF_BIN_WORK = 21,    /* uint32 per ray bin (8x8-pixel sub-tile; bin = 4 * (tileY * tilesX + tileX) + 2 * subY + subX over 16x16 tiles):
                                 lane-steps the last traversal spent on the bin's rays; zero unless that launch recorded them (full-size frames) */
  RTGGX_BUF_BVH4_TOP0 = 22,   /* the first (up to 16 / 96) 4-wide nodes of mesh 0 / 1 in breadth-first order, same 128-byte records; a reference to */
  RTGGX_BUF_BVH4_TOP1 = 23,   /*   a node that is in the table itself reads 0x40000000 | position (the copy the trace kernel keeps in LDS) */
  RTGGX_BUF_EXCHANGE_TOKENS = 24, /* 2 x RTGGX_MAX_PEERS uint32: words a multi-GPU host may send from ([rank]) and receive into ([RTGGX_MAX_PEERS + peer]) --
                                     the 4-byte messages that order two ranks without a neighbour's history rows between them (rtggx_set_history_peers) */
  RTGGX_BUF_ACC_REFL = 25,   /* 4 floats per pixel: sum r, sum g, sum b, sum Y^2 of RayTracingOut0 over the accumulated frames (rtggx_set_accumulation) */
  RTGGX_BUF_ACC_DIFF = 26,   /* the same of RayTracingOut1, where a diffuse path contributed; zero elsewhere */
  RTGGX_BUF_CONVERGED = 27,  /* uint64  R16G16B16A16_FLOAT, the mean image of the most recent rtggx_present_accumulation */
  RTGGX_BUF_COUNT = 28
};

/* Per-pass GPU timings of the last completed frame, in milliseconds (hipEvent based). */
typedef struct RtggxTimings {
  float update_as, visibility, ray_trace, spatial_refl_h, spatial_refl_v, spatial_diff_h, spatial_diff_v,
        temporal, tone_map, frame,
        ray_trace_kernel;   /* the fused raygen/trace/shade kernel alone (events right around its launch) */
} RtggxTimings;

const char* rtggx_last_error(void);

/* Creates a context on HIP device `device` with all render targets of RayTracer::Init and
 * Denoiser::Init for a width x height viewport.  The ground mesh of createGroundMesh and the
 * default materials are installed. */
int  rtggx_create(rtggx_context** out, uint32_t width, uint32_t height, int device);
void rtggx_destroy(rtggx_context* ctx);

/* Restrict rendering to the row strip [row_begin, row_end) of the full frame (multi-GPU screen
 * tiling); buffers stay full-size, rows outside the strip (plus the apron the
 * filters need) are not touched.  Default: the whole frame. */
int  rtggx_set_strip(rtggx_context* ctx, uint32_t row_begin, uint32_t row_end);

/* Strips only.  The temporal pass reprojects last frame's TemporalSSOut; rows next to a strip edge come from the neighbouring
 * rank, which the caller delivers between frames (`rows` beyond each edge; default 18 = 16 px of vertical motion per frame +
 * the bilinear tap + the pass's own 1-row apron).  rtggx_history_overreach returns the largest number of rows by which a
 * history tap read BEYOND the delivered rows since the last reset (0: every frame equals the single-GPU frame); synchronises. */
int  rtggx_set_history_apron(rtggx_context* ctx, uint32_t rows);
int  rtggx_history_overreach(rtggx_context* ctx, uint32_t* rows, int reset);

/* Make an externally owned hipStream_t the context's MAIN stream: shading, denoise and tone map run on it, and
 * every result the caller may read (traced images, filtered images, back buffer) is produced in its order.  The
 * visibility pass, ray generation and traversal keep running ahead on the context's internal stream B, joined
 * to the main stream by events.  NULL (also the handle of the null stream) restores the context's own stream. */
int  rtggx_set_stream(rtggx_context* ctx, void* hip_stream);
/* The context's main stream (its own, or the one handed in): what a host enqueues there -- the per-frame RCCL exchange of the
 * multi-GPU host, host/Strips.cpp -- is ordered behind the frame's tone map and before the next frame's temporal pass. */
int  rtggx_get_stream(rtggx_context* ctx, void** hip_stream);
/* Multi-GPU strips: history taps beyond the exchanged apron read the OWNER's image (round 4).  The reference samples its one history
 * texture anywhere (CSTemporalSS.hlsl:259-265); a rank holds last frame's TemporalSSOut for its own rows and `apron` rows either side.
 * With the other ranks' two history images mapped into this process the temporal pass reads a tap beyond those rows from the image of
 * the rank whose strip holds the row: N strips equal the single-GPU frame at any velocity (rtggx_history_overreach keeps counting such
 * taps; they are harmless then).
 *   bounds      world + 1 ascending rows: rank r owns [bounds[r], bounds[r + 1]) -- every rank allocates full-size targets, so a row sits
 *               at the same offset in every rank's image
 *   tss0, tss1  world device pointers each, valid in THIS process: rank r's TemporalSSOut[0] / [1] (rtggx_buffer_ptr of a context in
 *               the same process, or rtggx_history_ipc_open of another process's export); this rank's own entries may be null
 *   world = 0   forget the peers
 * Ordering is the caller's: rank A's temporal pass of frame f + 1 may read rank B's image once B's temporal pass of frame f has ended,
 * and B's horizontal filter of frame f + 2 -- which reuses that image as its scratch -- must wait for A's temporal pass of frame f + 1.
 * A per-frame exchange on the main streams (rtggx_get_stream) with a message in EACH direction between every two ranks orders both:
 * the neighbours' history rows do between neighbours, host/Strips.cpp and strips.py add 4-byte tokens between the other pairs. */
#define RTGGX_MAX_PEERS 16
#define RTGGX_IPC_HANDLE_BYTES 64
int  rtggx_set_history_peers(rtggx_context* ctx, uint32_t world, const uint32_t* bounds, void* const* tss0, void* const* tss1);
/* One process per GPU: this context's two history images as inter-process handles (2 x RTGGX_IPC_HANDLE_BYTES: hipIpcMemHandle_t of
 * TemporalSSOut[0], [1]; `bytes` = the room at `handles`) ... */
int  rtggx_history_ipc_export(rtggx_context* ctx, void* handles, size_t bytes);
/* ... and another process's handles opened in this one: two device pointers for rtggx_set_history_peers (unmapped by rtggx_destroy).
 * (HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of both processes on hosts whose driver only supports dmabuf IPC.) */
int  rtggx_history_ipc_open(rtggx_context* ctx, const void* handles, size_t bytes, void** tss0, void** tss1);

/* The sample's asynchronous-compute toggle (m_asyncCompute, key [A]: RayTracedGGX.cpp:304-353 issues the frame over two
 * queues, :513-556 as one command list).  enable = 0: every pass is issued to the main stream in submission order (no
 * stream B / C, no overlap between frames); 1 (default): the multi-stream frame.  Results are bit-identical; synchronises. */
int  rtggx_set_async_compute(rtggx_context* ctx, int enable);

/* Vertex = {float3 Pos; float3 Nrm} (24 bytes), 32-bit indices, triangle list of at most 2^24 triangles (a primitive id has 24 bits;
 * a larger mesh is refused and the slot keeps what it held). */
int  rtggx_set_mesh(rtggx_context* ctx, uint32_t slot, const float* verts, uint32_t num_verts,
                    const uint32_t* indices, uint32_t num_indices);
/* Cube map: `size` x `size` faces, `mips` levels, `data` laid out as in a DDS file (face-major,
 * full mip chain per face, faces +X -X +Y -Y +Z -Z).  BC6H blocks are decoded on the device. */
int  rtggx_set_env(rtggx_context* ctx, int format, uint32_t size, uint32_t mips, const void* data, size_t bytes);
/* Environments from images (no counterpart in the reference, whose probes were converted to BC6H cubes offline; DESIGN.md "Environments
 * from images"): the cube and its whole mip chain built on the device from a cross or a latitude-longitude panorama.  A context that calls
 * neither function allocates and launches what it always did.
 *   - data: width x height pixels, rows top to bottom, RTGGX_PIXELS_RGBE8 (4 bytes r, g, b, e: e == 0 is black, otherwise
 *     m 2^(e - 136) per channel) or RTGGX_PIXELS_RGB32F (3 floats).  Per channel v = x > 0 ? min(x, 65504) : 0: NaN and negatives become 0;
 *   - a cross (RTGGX_ENV_VCROSS: 3 x 4 square cells, RTGGX_ENV_HCROSS: 4 x 3) is never resampled: level 0 is a copy of six cells, cell
 *     (row, col) -> face; vertical: (0,1) +Y, (1,0) -X, (1,1) +Z, (1,2) +X, (2,1) -Y, (3,1) -Z turned by 180 degrees; horizontal: (0,1) +Y,
 *     (1,0) -X, (1,1) +Z, (1,2) +X, (1,3) -Z, (2,1) -Y.  cube_size must be 0; a cell above 4096 is refused;
 *   - a panorama (RTGGX_ENV_EQUIRECT, at most 16384 x 8192): cube_size 0 = the largest power of two <= width / 4, else any side from 1 to
 *     4096.  Per cube texel: d = the normalised direction through its centre, lon = atan2(d.x, d.z), lat = asin(d.y),
 *     s = (lon / 2 pi + 0.5) width - 0.5, t = (0.5 - lat / pi) height - 0.5 (+Z in the middle of the image, +X to its right, +Y in the
 *     top row), one bilinear tap at (s, t), columns wrapping and rows clamping; coordinates and weights in fp64, rounded to fp32 once;
 *   - the chain, for any side: floor(log2(size)) + 1 levels of side max(size >> m, 1), each face alone, separable, horizontal pass first.
 *     One axis from a parent side p to q = p >> 1, child i: p even (t[2i] + t[2i+1]) / 2; p odd ((q - i) t[2i] + q t[2i+1]) + (i + 1) t[2i+2],
 *     then / p -- the box of exact coverage.  Integer weights converted to float, every operation fp32 and rounded on its own in the order
 *     written; level m + 1 from the fp32 level m, not from its halves; every level packed to RGBA16F once, alpha 1.  RTGGX_BUF_ENV can be
 *     restated bit for bit (tests/envimage_ref.py);
 *   - refused, the context keeping the environment it had: null data, too few bytes, a width or height of 0, a source that is too large, a
 *     cross whose sides do not divide into square cells, an unknown layout or pixel format, cube_size with a cross or above 4096.
 * rtggx_generate_env_mips: the full chain below the CURRENT level 0 by the same rule -- level 0 widened from its halves (exact) and left
 * as it is, whatever levels the cube had below it replaced; fails when no environment is set.  For a cube uploaded with fewer levels than
 * a full chain: the shader picks a level from the roughness and clamps it to the last one there is.
 * Both synchronise, end the still-sky runs and invalidate the SH coefficients as rtggx_set_env does; the scratch is freed on return. */
enum { RTGGX_ENV_EQUIRECT = 0, RTGGX_ENV_VCROSS = 1, RTGGX_ENV_HCROSS = 2 };
enum { RTGGX_PIXELS_RGBE8 = 0, RTGGX_PIXELS_RGB32F = 1 };
int  rtggx_set_env_image(rtggx_context* ctx, int layout, int pixels, uint32_t width, uint32_t height, const void* data, size_t bytes,
                         uint32_t cube_size);
int  rtggx_generate_env_mips(rtggx_context* ctx);
/* GGX-prefiltered environments (opt-in, no counterpart in the reference, whose cubes were filtered offline; DESIGN.md "Prefiltered
 * environments"): the levels below level 0 rebuilt so that level m holds the radiance convolved with the GGX lobe of the roughness that
 * selects m -- what the split-sum shading at the end of a path (reflectionDepth1: environment(dir, level) x EnvBRDFApprox) assumes, and a
 * box chain is not.  A context that never calls it allocates and launches exactly what it always did.  samples: N, a power of two from
 * RTGGX_ENV_FILTER_MIN_SAMPLES to RTGGX_ENV_FILTER_MAX_SAMPLES, or 0 = 1024.  With S the cube's side and M = floor(log2 S) + 1:
 *   - source: the cube C that rtggx_generate_env_mips would leave now -- the current level 0 and below it the full box chain, RGBA16F.  The
 *     result depends on the current level 0 and on N alone: calling twice gives the same cube bit for bit; level 0 of the result is C's;
 *   - roughness of level m = 1 .. M - 1, in double: r = min(1.0, exp2((m - (M - 4)) / 1.15)) (the inverse of calcCubemapMipFromRoughness
 *     with M levels), a = r r, a2 = a a;
 *   - sample table of level m, built on the host, every expression a double operation in the order written with libm sqrt, cos, sin, log2,
 *     exp2 and pi = 3.14159265358979323846.  For i = 0 .. N - 1:
 *         u = bitreverse32(i) / 4294967296.0;  c2 = (1 - u) / (1 + (a2 - 1) u);  z = 2 c2 - 1     -- N.L with N = V = R;
 *     the entry is dropped unless z > 0; for the others
 *         ct = sqrt(c2);  st = sqrt(1 - c2);  phi = 2.0 pi (double)i / (double)N;  x = 2 ct st cos(phi);  y = 2 ct st sin(phi);
 *         d = (a2 - 1) c2 + 1;  pdf = a2 / (pi d d) / 4;  lod = 0.5 log2((6.0 S S) / (4 pi N pdf)) + 1.0;  lod = min(max(lod, 0), M - 1).
 *     The K kept entries stay in order of i, each ((float)x, (float)y, (float)z, (float)lod); invW = (float)(1.0 / sum of (double)(float)z),
 *     in that order.  Entry i = 0 is always kept (z = 1); at r = 1 -- every level m >= M - 4 -- exactly the even i are, K = N / 2;
 *   - texel (face f, x, y) of level m, side s = max(S >> m, 1), everything fp32 without contraction, each operation rounded on its own:
 *         u = ((float)x + 0.5f) / (float)s * 2.0f - 1.0f, v likewise;  R = normalize(cubeFaceDir(f, u, v));
 *         term_k = environment(C, localToWorld(R, (x_k, y_k, z_k)), lod_k) * z_k per component
 *     -- the sampler and the tangent frame of the frame's kernels (rtggx_debug_environment; RayTracing.hlsl:129-147, 167-180);
 *   - THE ORDER OF THE SUM IS FIXED: 64 partials p_j = ((+0 + term_j) + term_{j+64}) + ... over k = j (mod 64) ascending (+0 where there is
 *     none), added pairwise, adjacent pairs first: q[i] = p[2 i] + p[2 i + 1], level by level, six levels, to t.  The texel is
 *     pack_rgba16f(min(t.r invW, 65504), min(t.g invW, 65504), min(t.b invW, 65504), 1).  No atomics, no order that depends on
 *     scheduling: tests/envfilter_ref.cpp restates RTGGX_BUF_ENV bit for bit.  A cube with negative or non-finite texels: not specified.
 * Refused, the context keeping its environment, still-sky runs and frame: no environment set; samples neither 0 nor a power of two in
 * range.  Otherwise like rtggx_generate_env_mips: synchronises, builds the new cube beside the old one and installs it when everything
 * has succeeded, ends the still-sky runs, invalidates the SH coefficients, frees its scratch on return. */
#define RTGGX_ENV_FILTER_MIN_SAMPLES 64u
#define RTGGX_ENV_FILTER_MAX_SAMPLES 4096u
int  rtggx_prefilter_env(rtggx_context* ctx, uint32_t samples);   /* 0 = 1024 */
int  rtggx_set_material(rtggx_context* ctx, uint32_t mesh, const float base_color[4], float roughness, float metallic);
int  rtggx_set_metallic(rtggx_context* ctx, uint32_t mesh, float metallic);
/* Sampler of the reflection lobe.  0 (default): the reference's -- the GGX normal distribution itself, computeLocalDirectionGGX /
 * computeReflection (RayTracing.hlsl:92-101, 129-147, 424-484), weight NoL F Vis 4 VoH / NoH -- the parity path.  1: the distribution
 * of VISIBLE normals (Heitz 2018), weight F G1(L): no sample is wasted below the horizon of the view direction, less variance at
 * grazing angles for the same one sample per pixel.  Takes effect with the next rtggx_update_frame. */
int  rtggx_set_sampler(rtggx_context* ctx, int vndf);
/* Ray rate: pixels per traced ray, 1 (default: every covered pixel traces its reflection ray, and its diffuse ray where metallic < 1 --
 * DispatchRays(W,H,1) of the reference) or 4 (opt-in, no counterpart in the reference; DESIGN.md "Quarter-rate tracing"):
 *   - traced pixel: with F = FrameIndex & 3 and o = {(0,0), (1,1), (1,0), (0,1)}[F], pixel (x, y) traces iff (x & 1, y & 1) == o --
 *     every pixel once in any four consecutive frames (FrameIndex wraps at 256).  Its RayTracingOut0/1 words are bit-identical to the
 *     full-rate frame's (same sample, ray and shading);
 *   - at every pixel as at rate 1, bit for bit: visibility, depth, normal, rough/metal, velocity, and background pixels (environment
 *     along -V, no ray);
 *   - an untraced covered pixel c is reconstructed before the spatial filters from the traced pixels q at Chebyshev distance 1 that
 *     are covered by c's instance: RayTracingOut0 = sum w L(q) / sum w with w = NormalWeight(nc, nq, 32) DepthWeight(zc, zq, 4)
 *     RoughnessWeight(rc, rq, 0, 0.5) (FilterCommon.hlsli:34-47 on the G-buffer words); RayTracingOut1, where c's metallic < 1, with
 *     w = NormalWeight(nc, nq, 32) DepthWeight(zc, zq, 4).  sum w = 0: the plain mean of those q; none: the plain mean of c's instance's
 *     traced pixels within distance 2; none: 0.  Where metallic >= 1 RayTracingOut1 keeps what it held, as at rate 1;
 *   - rtggx_ray_count / rtggx_ray_total count the rays traced.
 * Whole frames only: rate 4 on a context with a strip (rtggx_set_strip), and a strip on a rate-4 context, are refused.  Takes effect
 * from the next rtggx_render_visibility; synchronises. */
int  rtggx_set_ray_rate(rtggx_context* ctx, uint32_t pixels_per_ray);
/* Recursion depth (RayTracer::SetMaxRecursionDepth; RayTracer.cpp:605 and RayTracing.hlsl:11 fix it at 1): D levels of rays per path,
 * 1 (default: the reference's renderer, bit for bit) to RTGGX_MAX_RECURSION_DEPTH; anything else is refused and the depth kept.  Depth D is
 * the reference's shaders with the closest hits passing payload.RecursionDepth + 1 (DESIGN.md "Recursion depth").  For the reflection path
 * and the diffuse path of a pixel:
 *   - level 0 is the depth-1 frame's: the ray, its weight w0, the G-buffer, the background, NoL <= 0 -> 0;
 *   - a level-d ray carries the throughput T_d: T_0 = w0, T_{d+1} = T_d * w_{d+1} per component (fp32); the pixel's word is
 *     pack_r11g11b10(c * T) with c the value at the end of the path (the throughput is multiplied forward, not on the way back);
 *   - a miss ends the path with c = environment(dir, level 0);
 *   - a hit of a level-d ray with d + 1 == D ends it with the depth-1 shading: reflectionDepth1, or SH irradiance / pi x colour;
 *   - a hit with d + 1 < D follows closestHitReflection / closestHitDiffuse (:571-614) at depth d + 1: a reflection-group ray whose
 *     preset (colour x metallic of the surface it left) is <= 0 in every component ends with c = preset; else, with P = o + t dir (fp32,
 *     per component), V = -dir and the surface's normal and material, metallic > 0.5: computeReflection with the PIXEL's xi
 *     (getSampleParam(DispatchRaysIndex())) at every level, GGX or VNDF (rtggx_set_sampler), R = reflect(-V, H); NoL <= 0 ends the path
 *     with c = 0, else a reflection-group ray from P along R (skip: the hit's (inst << 24) | prim; interval (1e-5, 1e4)) of weight
 *     ((NoL F) vis) k, or F G1(L) with VNDF; otherwise computeDiffuse: a diffuse-group ray multiplies the colour by (1 - metallic) (:607),
 *     and a diffuse-group ray along normalize(N + uniformSphere(xi)) follows with weight = that colour (no x 0.96 at depth >= 1, :532);
 *   - the image a path writes, RayTracingOut0 or RayTracingOut1, is its level-0 ray's;
 *   - rtggx_ray_count / rtggx_ray_total count the rays of every level, RtggxTimings.ray_trace covers every level, ray_trace_kernel is
 *     the level-0 traversal.
 * Works with quarter-rate tracing (only traced pixels start paths) and on strips.  Takes effect from the next rtggx_render_visibility. */
#define RTGGX_MAX_RECURSION_DEPTH 4u
int  rtggx_set_max_recursion_depth(rtggx_context* ctx, uint32_t depth);
/* Samples per pixel (RayTracer::SetSamplesPerPixel; the reference traces one): N = 1 (default: the reference's renderer, bit for bit), 2, 4
 * or RTGGX_MAX_SAMPLES_PER_PIXEL; anything else is refused and the setting kept (DESIGN.md "Samples per pixel").
 *   - at every pixel as at N = 1, bit for bit: visibility, depth, normal, rough/metal, velocity; background pixels (the environment along
 *     -V, no ray and no averaging); RayTracingOut1 where metallic >= 1 (it keeps what it held);
 *   - sample k = 0 .. N - 1 of a covered pixel is the one-sample frame's level-0 code -- computeReflection / computeDiffuse at depth 0, GGX
 *     or VNDF (rtggx_set_sampler) -- with xi = getSampleParam(pixel, FrameIndex * N + k) in place of getSampleParam(pixel, FrameIndex)
 *     (not wrapped: FrameIndex < 256).  At recursion depth D the whole path of D levels carries that sample's xi at every level, the
 *     throughput multiplied forward as at N = 1.  So the samples of frame F are exactly those of N consecutive one-sample frames with the
 *     frame indices F * N .. F * N + N - 1, and consecutive frames never repeat a sample inside the 256-frame period;
 *   - the pixel's word, per image and component, in fp32 without contraction: acc = 0, then acc = acc + v_k for k = 0, 1, ..., N - 1 in
 *     that order, v_k = c_k * T_k the value a one-sample frame packs (0 where sample k traces nothing: NoL <= 0); the word is
 *     pack_r11g11b10(acc * (1 / N)) -- N is a power of two, the scaling exact.  RayTracingOut1 likewise where the pixel's metallic < 1.
 *     No atomics and no order that depends on scheduling: the image is a pure function of the inputs;
 *   - rtggx_ray_count / rtggx_ray_total count the rays of every sample and level, RtggxTimings.ray_trace covers all of them,
 *     ray_trace_kernel is the first sample's level-0 traversal.
 * Works at every recursion depth, with both samplers, on strips and with a deforming mesh.  N > 1 on a context at ray rate 4, and rate 4 on
 * a context with N > 1, are refused (one asks for more rays, the other for fewer) and the context keeps what it had.  The first N > 1
 * allocates 24 bytes per pixel of the full frame, released by rtggx_destroy.  Takes effect from the next rtggx_render_visibility. */
#define RTGGX_MAX_SAMPLES_PER_PIXEL 8u
int  rtggx_set_samples_per_pixel(rtggx_context* ctx, uint32_t samples);
/* Sample-set size (RayTracer::SetSampleSetSize; the reference's shader declares getSampleParam(index, dim, numSamples = 256) and never
 * passes another size): M = RTGGX_MIN_SAMPLE_SET (default: the reference's renderer, bit for bit) or a power of two up to
 * RTGGX_MAX_SAMPLE_SET; anything else is refused and the context keeps what it had (DESIGN.md "Sample-set size").
 *   - the sample with index i at pixel (x, y) of a frame W pixels wide: s = rng(rng(y W + x) + i) & (M - 1); xi.x = s / M;
 *     xi.y = (rng(s) & 0xffff) / 65536; (cosPhi, sinPhi) = ((float)cos(phi), (float)sin(phi)) with
 *     phi = 2.0 * 3.14159265358979323846 * (double)s / (double)M -- double libm, rounded once: the table rule of the 256-member set with M
 *     in place of 256, so entry k M / 256 of the M-table equals entry k of that one;
 *   - i is what it is at M = 256: FrameIndex at one sample per pixel, FrameIndex * N + k at N samples; the same pixel's xi at every level of
 *     a path of depth D; both samplers, GGX and VNDF (rtggx_set_sampler), take it;
 *   - nothing else of a frame depends on M: G-buffer, visibility, background words, still-sky runs, tile words, the rate-4 pattern
 *     (FrameIndex & 3) and the denoiser;
 *   - the caller's FrameIndex should count modulo M (RayTracer::UpdateFrame does): the library does not wrap it.  With a still camera the
 *     frames then repeat after M instead of 256, and an accumulation converges that much further;
 *   - works at every recursion depth and sample count, at ray rate 4, on strips, with a deforming mesh, accumulation and a still sky.  It
 *     ends no still-sky run (a pixel without a surface takes no sample) and resets no accumulation: like a changed material that is the
 *     caller's to do.
 * Every size M > 256 allocates, the first time it is set, a table of 2 M floats (512 KB at 65536), released by rtggx_destroy; a context that
 * never calls this allocates and launches exactly what it always did.  Takes effect from the next rtggx_render_visibility; synchronises --
 * and where that rtggx_render_visibility renders from the constants of an earlier frame (no rtggx_update_frame in between) it waits for that
 * frame first. */
#define RTGGX_MIN_SAMPLE_SET 256u
#define RTGGX_MAX_SAMPLE_SET 65536u
int  rtggx_set_sample_set(rtggx_context* ctx, uint32_t size);
/* Progressive accumulation (opt-in, no counterpart in the reference; DESIGN.md "Progressive accumulation"): the long-run mean of the
 * denoiser's INPUT, kept on the device.  Off (default): nothing is allocated and a frame launches what it always did.  enable = 1 takes
 * effect from the next rtggx_render_visibility; the first one allocates 2 x 16 + 8 bytes per pixel of the full frame, zeroed, released by
 * rtggx_destroy.  Enabling does not reset; disabling keeps the sums and the count.
 *   - while on, every rtggx_ray_trace ends with one more kernel on the main stream, behind the hit shading and the sample resolve and in
 *     front of rtggx_denoise (RtggxTimings.ray_trace covers it), and the frame count n grows by one.  For every pixel of the context's own
 *     rows [row_begin, row_end) -- no apron --, in fp32 without contraction, one lane per pixel, no atomics, frames in main-stream order:
 *         (r, g, b) = unpack_r11g11b10(RayTracingOut0);  A0.xyz += (r, g, b);  Y = (0.25 r + 0.5 g) + 0.25 b;  A0.w += Y * Y
 *     -- background pixels too: they hold the environment --, and the same into A1 from RayTracingOut1 where the pixel is covered and its
 *     instance's metallic in that frame's constants is < 1 (elsewhere RayTracingOut1 holds a carry-over nobody reads, and A1 is not
 *     touched).  Non-finite words add as they are.  The sums are a pure function of the frames: RTGGX_BUF_ACC_REFL / _DIFF can be restated
 *     bit for bit from the frames' words (tests/accum_ref.py);
 *   - the sums exist once, not per input set.  A moving camera or a changed material is the caller's to reset:
 *     rtggx_reset_accumulation zeroes the sums and the count, enqueued on the main stream without waiting;
 *   - rtggx_accumulated_frames: n.  With a still camera the sequence of frames repeats after 256: the sample set of the reference has 256
 *     members (getSampleParam) and FrameIndex wraps there -- an accumulation cannot converge past the mean of those 256 (a larger set:
 *     rtggx_set_sample_set);
 *   - rtggx_present_accumulation (whole frames and n > 0; refused on a strip and at n = 0): per pixel and component
 *     m0 = (float)((double)A0.c / (double)n), m1 likewise, RTGGX_BUF_CONVERGED = pack_rgba16f(m0.r + m1.r, m0.g + m1.g, m0.b + m1.b, 1)
 *     with fp32 adds -- the denoiser's composition dest + diffuse of the two means, A1 being zero where no diffuse path ever contributed --,
 *     then the tone map of that image into RTGGX_BUF_BACKBUFFER.  Both on the main stream; the next frame's tone map overwrites the back
 *     buffer as always, and no other image is touched;
 *   - works with both samplers, every recursion depth and sample count (the word accumulated is the resolved one), a deforming mesh and on
 *     strips (rows outside the strip stay zero).  Three quarters of a rate-4 frame are interpolations: rtggx_set_accumulation(1) on a
 *     context at ray rate 4, and rate 4 on an accumulating context, are refused and the context keeps what it had;
 *   - rtggx_readback / rtggx_buffer_size / rtggx_buffer_ptr of RTGGX_BUF_ACC_REFL, _ACC_DIFF and _CONVERGED fail on a context that never
 *     enabled accumulation. */
int  rtggx_set_accumulation(rtggx_context* ctx, int enable);
int  rtggx_reset_accumulation(rtggx_context* ctx);
int  rtggx_accumulated_frames(rtggx_context* ctx, uint32_t* frames);
int  rtggx_present_accumulation(rtggx_context* ctx);

/* Scoring against a reference image (opt-in, no counterpart in the reference; DESIGN.md "Scoring against a reference"): every frame's
 * distance from a reference image, reduced on the device inside the frame, the records collected by the host whenever it likes.  A
 * context that never calls any of the four functions below allocates and launches exactly what it always did.
 *   - rtggx_set_reference: W * H RGBA16F words (`bytes` = W * H * 8, anything else is refused), the layout rtggx_readback of
 *     RTGGX_BUF_CONVERGED gives; the alpha half is not read.  Synchronises and copies before it returns; may replace a reference in
 *     mid-run.  (NULL, 0) releases the image and turns scoring off.  The first call allocates 8 bytes per pixel of the full frame;
 *   - rtggx_reference_from_accumulation: the reference becomes the mean image rtggx_present_accumulation computes -- same arithmetic,
 *     on the main stream, no wait -- without touching RTGGX_BUF_CONVERGED or the back buffer.  Whole frames and n > 0, as there;
 *   - rtggx_set_scoring(1) is refused without a reference.  It takes effect from the next rtggx_render_visibility; the first enable
 *     allocates the ring of RTGGX_SCORE_RING records and the tree's partial sums (about 108 bytes per 1024 pixels of the full frame);
 *   - while scoring is on, rtggx_denoise ends with two more kernels on the main stream, behind the temporal pass and in front of the tone
 *     map, which then always runs as a kernel of its own (as in the per-pass timing mode; the images are the same either way).  They
 *     write one RtggxScore into slot index % RTGGX_SCORE_RING of the ring;
 *   - rtggx_read_scores waits for the main stream only and copies the unread records, oldest first, up to `capacity`; the rest stay
 *     unread.  When more than RTGGX_SCORE_RING frames were scored since the last read the oldest are gone: the gap in `index` shows it.
 * Per pixel of the context's own rows [row_begin, row_end) -- no apron --, every quantity converted to double (exact) and every operation
 * a double operation rounded on its own (no contraction):
 *     ref = the reference's rgb;   out = the rgb of TemporalSSOut[parity] of the frame just denoised;
 *     raw = unpack_r11g11b10(RayTracingOut0) + (diff ? unpack_r11g11b10(RayTracingOut1) : nothing), diff as in rtggx_set_accumulation:
 *           the pixel is covered (visibility word != 0) and its instance's metallic in that frame's constants is < 1;
 *     Y(c) = (0.25 c.r + 0.5 c.g) + 0.25 c.b;   E(c) = (c.r c.r + c.g c.g) + c.b c.b;
 *     se_out_rgb += E(out - ref), se_out_luma += (Y(out) - Y(ref))^2, ref_rgb2 += E(ref), ref_luma2 += Y(ref)^2 -- unless a component
 *     of out or ref is not finite: then the pixel adds +0.0 to these four and to the three *_cov sums' out and ref terms, and counts
 *     in skipped_out;  se_raw_rgb += E(raw - ref), se_raw_luma += (Y(raw) - Y(ref))^2 -- unless a component of raw or ref is not finite:
 *     +0.0 and skipped_raw;  se_out_rgb_cov, se_raw_rgb_cov, ref_rgb2_cov: the terms of se_out_rgb, se_raw_rgb, ref_rgb2 where the
 *     pixel is covered, +0.0 elsewhere.
 * THE ORDER OF EVERY SUM IS FIXED.  The P pixels of the context's own rows are numbered p = 0 .. P - 1, row-major from row_begin; the
 * sequence of a sum's terms is padded with +0.0 to the next power of two and added pairwise, adjacent pairs first: x[2 i] + x[2 i + 1],
 * level by level, until one value is left (P = 0: +0.0).  The result depends on P and on nothing else -- not on the grid, the workgroup
 * size, the stream placement or how many pixels a lane takes; tests/score_ref.py restates it bit for bit.  Counts are integers.
 * Works at every ray rate (4 included), with both samplers, every depth, sample count and sample-set size, a deforming mesh, a
 * caller-owned stream, rtggx_set_async_compute(0) and on strips: a strip scores its own rows, and adding the strips' records is the
 * caller's.  Refusals (wrong `bytes`, scoring without a reference, null results) leave the context as it was. */
typedef struct RtggxScore {            /* 120 bytes (6 x 8 of counts, 9 x 8 of sums), all sums in fp64 */
  uint64_t index;        /* frames scored by this context before this one (monotonic over off/on): a gap = records overwritten unread */
  uint32_t frame_index;  /* RtggxCBGlobal::FrameIndex of the scored frame */
  uint32_t pad;
  uint64_t pixels, covered;            /* the context's own rows x W; of those, visibility word != 0 */
  uint64_t skipped_out, skipped_raw;   /* pixels left out of the *_out / *_raw sums: a non-finite rgb component in the image or the reference */
  double se_out_rgb, se_out_luma;      /* TemporalSSOut[parity] against the reference, all pixels */
  double se_raw_rgb, se_raw_luma;      /* the raw frame against the reference, all pixels */
  double ref_rgb2, ref_luma2;          /* the reference's own energy over the pixels of the *_out sums */
  double se_out_rgb_cov, se_raw_rgb_cov, ref_rgb2_cov;   /* covered pixels only */
} RtggxScore;
enum { RTGGX_SCORE_RING = 256 };
int  rtggx_set_reference(rtggx_context* ctx, const void* rgba16f, size_t bytes);
int  rtggx_reference_from_accumulation(rtggx_context* ctx);
int  rtggx_set_scoring(rtggx_context* ctx, int enable);
int  rtggx_read_scores(rtggx_context* ctx, RtggxScore* out, uint32_t capacity, uint32_t* count);

/* Adaptive sampling (opt-in, no counterpart in the reference; DESIGN.md "Adaptive sampling"): with N > 1 samples per pixel
 * (rtggx_set_samples_per_pixel) a map says how many of the N samples each 8 x 8-pixel block of the full frame traces.  A context that never
 * calls either of the two functions below allocates and launches exactly what it always did.
 *   - the map: one count per block, row-major, blocks_x = ceil(W / 8) by blocks_y = ceil(H / 8), each count 1, 2, 4 or 8.  A block is one ray
 *     bin -- one wave of ray generation --, and the device copy is kept in bin order (RTGGX_BUF_BIN_WORK's: bin = 4 tile + 2 subY + subX);
 *   - with c = min(count of the pixel's block, N): a covered pixel traces the samples k = 0 .. c - 1 of the N-sample frame -- the same
 *     samples, indices FrameIndex * N + k, at every recursion level, with both samplers and every sample-set size --, and its word is
 *     pack_r11g11b10((0 + v_0 + ... + v_{c-1}) * (1 / c)) in fp32, in that order, without contraction; RayTracingOut1 likewise where the
 *     pixel's metallic < 1.  Everything else is the N-sample frame's bit for bit: G-buffer, visibility and background words, the carry-over
 *     of RayTracingOut1 at metallic >= 1, tile words, still-sky and settled-sky behaviour, accumulation (it adds the resolved word) and
 *     scoring.  A map of all N, or no map, is the N-sample frame; a map of all 1 holds at covered pixels the words of a one-sample frame
 *     with FrameIndex * N as its index;
 *   - rtggx_ray_count / rtggx_ray_total count the rays actually traced.  The frame still launches the N * D passes of the N-sample frame:
 *     a wave whose block has had its c samples stores an empty bin and leaves, and the traversal and shading passes find fewer rays;
 *   - N = 1 ignores the map: the one-sample frame launches what it always did;
 *   - rtggx_set_sample_map(ctx, NULL, 0, 0) clears the map.  Refused, the context keeping what it had: other dimensions than the frame's,
 *     a count other than 1, 2, 4 or 8, a map on a context with a strip and a strip on a context with a map (strip tiles count from the
 *     pass's first row, so a block would no longer be a bin: whole frames only, like ray rate 4).  Synchronises; takes effect from the
 *     next rtggx_render_visibility.  The first set allocates 2 x 4 bytes per 16 x 16 tile, released by rtggx_destroy;
 *   - rtggx_read_sample_map: the map most recently set, row-major, read back from the device copy; blocks_x = blocks_y = 0
 *     and nothing written when there is none.  A capacity below blocks_x * blocks_y is refused (the dimensions are still returned).
 *     Synchronises.
 * The library sets no policy: where the counts come from is the caller's (DESIGN.md "Adaptive sampling" records the one that was measured
 * and left out).  tests/adaptive_ref.py restates the frames. */
int  rtggx_set_sample_map(rtggx_context* ctx, const uint8_t* counts, uint32_t blocks_x, uint32_t blocks_y);
int  rtggx_read_sample_map(rtggx_context* ctx, uint8_t* counts, uint32_t capacity, uint32_t* blocks_x, uint32_t* blocks_y);

/* Build of both bottom-level structures (RayTracer::buildAccelerationStructures / BuildAccelerationStructures, RayTracer.cpp:676-716,
 * 158-233; the sample records the builds on the GPU timeline and waits once, RayTracedGGX.cpp:236): every step of the build --
 * Morton codes, sort, PLOC clustering, the refit schedule, the node arrays -- is a kernel launch on the context's build stream
 * with no host round trip between them; the call waits once, at the end. */
int  rtggx_build_as(rtggx_context* ctx);

/* Deforming mesh: `num_verts` new vertices (same layout, same count, same indices as the last rtggx_set_mesh) for mesh `slot`.
 * Replaces, for shape changes, what RayTracer::UpdateAccelerationStructure (RayTracer.cpp:326-341) does for the rigid instance
 * motion of the sample: the acceleration structure follows the new positions without a synchronisation.
 * The vertices are copied (staged) before the call returns; the upload, the new leaf triangles and the bottom-up box refit of
 * the existing tree run on the context's refit stream at the start of the next frame (rtggx_render_visibility), overlapping the
 * previous frame's shading and denoising.  A refit keeps the topology of the last build; when the refitted tree's cost exceeds
 * `rebuild_ratio` x that of the last build (rtggx_set_refit_policy, default 1.2), the mesh is REBUILT from its newest shape beside
 * the frames: `steps_per_frame` kernel launches of the build per frame (default 16; ~75 for the bunny) behind that frame's refit,
 * the new topology taking over between two frames when the last one has ended.  Neither call waits for the GPU (the first
 * rtggx_refit_as of a mesh allocates its per-set buffers).  While a mesh deforms on a full-size frame the context keeps three frames in
 * flight instead of four (rtggx_render_visibility waits for the end of frame f - 3): one frame time instead of two, DESIGN.md section 9.
 * rtggx_refit_stats: cost of the current tree relative to the last
 * build, refits and rebuilds so far; synchronises (a rebuild in progress stays in progress).  A build whose cost is 0 -- one triangle, or
 * every vertex on one axis-aligned line or at one point -- reports 1 while the cost stays 0 and +infinity once it is not: any growth of
 * such a mesh asks for a rebuild. */
int  rtggx_refit_as(rtggx_context* ctx, uint32_t slot, const float* verts, uint32_t num_verts);
/* The same for a mesh animated ON the GPU (round 4): `device_verts` is a device pointer, `hip_stream` the stream that produces it (NULL: the
 * null stream).  Like a hipMemcpyAsync on that stream: the copy out of `device_verts` is ordered behind everything the stream holds at the
 * time of the call, and what the caller enqueues there afterwards (the next animation step) behind the copy; it runs on the context's
 * geometry stream into a device-side staging ring -- no host copy, no wait. */
int  rtggx_refit_as_device(rtggx_context* ctx, uint32_t slot, const float* device_verts, uint32_t num_verts, void* hip_stream);
int  rtggx_set_refit_policy(rtggx_context* ctx, float rebuild_ratio, uint32_t steps_per_frame);
int  rtggx_refit_stats(rtggx_context* ctx, uint32_t slot, float* cost_ratio, uint32_t* refits, uint32_t* rebuilds);

/* Per-frame constants; copied into the next slot of a ring of (input sets + 1) = 5. */
int  rtggx_update_frame(rtggx_context* ctx, const RtggxFrameConstants* constants);
/* Refreshes the TLAS (the two world->object matrices) from the constants of the current slot.  May be called before or
 * after rtggx_render_visibility of the same frame (the sample overlaps the two on different queues); rtggx_ray_trace sends
 * the refreshed constants to the device again when the visibility pass had already carried the slot there. */
int  rtggx_update_as(rtggx_context* ctx);
int  rtggx_transform_sh(rtggx_context* ctx);
/* Starts a frame: advances to the next of 4 input sets (G-buffer, traced images, ray bins, and -- for a deforming mesh -- vertices and
 * tree; the sample's RayTracer::FrameCount is 3).  All pass functions only enqueue work; this one is the frames-in-flight fence of the
 * sample (RayTracedGGX.cpp:672-701): it blocks the calling thread while the frame that last used that set, four frames back, is still
 * being read on the GPU.  A pending rtggx_refit_as is issued here. */
int  rtggx_render_visibility(rtggx_context* ctx);
int  rtggx_ray_trace(rtggx_context* ctx);
int  rtggx_denoise(rtggx_context* ctx, int use_shared_mem);
int  rtggx_tone_map(rtggx_context* ctx);

/* Round 4: rtggx_denoise's temporal pass can tone-map its result as well (one kernel instead of two: Denoiser::Denoise and ::ToneMap
 * follow each other in every frame of the sample, RayTracedGGX.cpp:341-350); the rtggx_tone_map that follows it in the same frame then
 * finds its work done.  The library does so where it pays: on small launches (thin strips, small frames), not on full-size frames
 * (measured: profiles/r04_c_pipeline_ab.txt).  A tone map without a preceding rtggx_denoise in the frame, or after an rtggx_upload,
 * always runs as a kernel of its own.  Diagnostic: mode 0 = always two kernels, 1 = always fused, -1 = the library's choice again;
 * the back buffer and TemporalSSOut are bit-identical either way. */
int  rtggx_debug_fuse_tone_map(rtggx_context* ctx, int mode);
/* Diagnostic: which streams a frame's kernels go to is decided from five facts (frame.hip placeFrame: small launch, strip, deforming
 * mesh, diffuse rays, caller-owned main stream).  force_small = 0 / 1 pins the first of them whatever the ray count says (-1: by the
 * count again).  key / where (may be null): the most recent rtggx_ray_trace's key (bit 0 small, 1 strip, 2 deforming, 3 diffuse,
 * 4 caller-owned stream) and placement (bits 0-3 / 4-7 / 8-11 / 16-19: stream of ray generation / traversal / hit shading / the visibility pass --
 * 0 main, 1 B, 2 C, 3 R --, bits 12-15 frames in flight).  Results do not depend on any of it. */
int  rtggx_debug_placement(rtggx_context* ctx, int force_small, uint32_t* key, uint32_t* where);
/* Diagnostic (round 4): the visibility pass keeps one word per 16x16 tile of its target -- "something was drawn here" -- and the kernels
 * behind it (ray generation, traversal, hit shading, the tiled spatial filters) leave a tile whose word is 0 after a scalar load instead of
 * fetching pixels to find that out; ray generation neither reads nor re-clears such a tile of the target (RayTracer.cpp:751-791 clears and
 * reads the whole target every frame).  enable = 0: every tile is treated as drawn, as in rounds 1-3.  Same images either way. */
int  rtggx_debug_tile_words(rtggx_context* ctx, int enable);
/* Diagnostic (still sky): per input set and 16x16 tile, ray generation counts the consecutive frames in which it found the tile's word 0
 * while nothing a sky pixel's outputs depend on changed (camera, environment, rows, uploads ...: an "epoch").  A tile whose run is long enough
 * holds, in that set, everything ray generation would store there, and is left alone; the reflection V pass leaves blocks alone whose sky
 * texels it converted into the same image the frame before.  enable = 0: the runs are counted and nothing is left alone.  Same images
 * either way. */
int  rtggx_debug_static_sky(rtggx_context* ctx, int enable);
/* ... and the current input set's runs under the current epoch, one word per tile of the most recent ray generation's grid (row-major,
 * *tiles_x by *tiles_y; capacity in words).  *threshold: the run from which that ray generation left a tile alone.  Synchronises. */
int  rtggx_debug_sky_runs(rtggx_context* ctx, uint32_t* runs, uint32_t capacity, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* threshold);
/* Diagnostic (settled sky): over sky that has stopped changing the temporal pass would store the bits it stored two frames ago and the tone
 * map the bits of the frame before.  The temporal pass keeps one word per 64x4 block, twice by history parity -- epoch << 8 | bit 0: every
 * texel the block computed equals the one in place in the other history image | bit 1: the block was left alone --, and leaves a block
 * alone whose window is sky and which was settled, with its eight neighbours, in the frame before; the tone map leaves a 64x16 block alone
 * over settled blocks.  Whole frames of the two-kernel path only.  enable = 0: no words, nothing left alone.  Same images either way. */
int  rtggx_debug_settled_sky(rtggx_context* ctx, int enable);
/* ... and both word arrays (array p belongs to TemporalSSOut[p]), *blocks_x columns of *blocks_y words each, column after column
 * (capacity in words, per array); *epoch: the epoch that words count under now.  Synchronises. */
int  rtggx_debug_settled_words(rtggx_context* ctx, uint32_t* words0, uint32_t* words1, uint32_t capacity, uint32_t* blocks_x, uint32_t* blocks_y, uint32_t* epoch);
/* Diagnostic: the two weights of the 4-wide collapse's objective (lbvh.hip "the 4-wide collapse"): a 4-wide node costs
 * area_weight x (its half-area / the root's) + tris_weight x (its triangles / all triangles) -- the chance that a random ray enters it,
 * and the chance that a ray STARTING on the mesh's surface (every ray of this path does) starts inside it.  set (may be null): weights for
 * builds from now on; get (may be null): the current ones.  Results do not depend on them. */
int  rtggx_debug_collapse_weights(rtggx_context* ctx, const float* set, float* get);
/* Diagnostic: the host time (us) rtggx_render_visibility has spent WAITING at the frames-in-flight fence -- for the last reader of the
 * input set it is about to overwrite, four frames back (RayTracedGGX.cpp:672-701) -- and how many frames had to wait, since the last reset.
 * A frame loop that is bound by the GPU waits there every frame; one that is bound by its own submission never does. */
int  rtggx_debug_fence_wait(rtggx_context* ctx, double* us_total, uint32_t* waits, int reset);

int  rtggx_sync(rtggx_context* ctx);
/* Number of non-degenerate rays (TMax > TMin) traced by the last rtggx_ray_trace; synchronises. */
int  rtggx_ray_count(rtggx_context* ctx, uint64_t* rays);
/* Rays traced since the last reset (accumulated on the device, no per-frame synchronisation); synchronises. */
int  rtggx_ray_total(rtggx_context* ctx, uint64_t* rays, int reset);
/* Diagnostic counters (non-zero only in builds with -DRT_TRACE_STATS): [0] lane node steps, [1] lane leaf steps,
 * [2] wave iterations, [3] refills of the trace kernel since the last reset. */
int  rtggx_debug_counters(rtggx_context* ctx, uint32_t* out, uint32_t n, int reset);
/* Tuning / test hook of the trace kernel's adaptive split (bins that were expensive in the previous frame are traced by
 * 2, 4 or 8 waves): work_per_wave = lane-steps of traversal per wave above which a bin is split further (0: never),
 * max_shift = log2 of the most waves per bin (0..3), capacity = room in the split list, in waves (-1: sized from the
 * demand of earlier frames, the default).  *last_demand (may be NULL) receives the number of list entries the most recent
 * frame asked for; synchronises.  Results do not depend on any of this: hits merge with a 64-bit atomic min. */
int  rtggx_debug_trace_split(rtggx_context* ctx, uint32_t work_per_wave, uint32_t max_shift, int capacity, uint32_t* last_demand);
/* The traversal kernel keeps one workgroup of 12 to 16 waves per CU resident on full-size frames; the size follows the share of
   the frame period the traversal takes (DESIGN.md "The trace kernel").  Reports the size and the share last sampled (0 before the
   first sample).  force_waves: 0 leaves the choice to the library, 10/12/14/16 pins it (measurement). */
int  rtggx_debug_trace_residency(rtggx_context* ctx, uint32_t force_waves, uint32_t* waves, float* share);
/* Diagnostic / test hook: the environment sampler alone.  rgb3[3 i ..] = the filtered cube map in direction dirs3[3 i ..] (any length but 0;
 * no NaN or infinity) at mip level levels[i] -- clamped to [0, mips - 1], trilinear --, computed on the device by the very functions ray
 * generation and hit shading call (D3D cube sampling restated: DESIGN.md).  level0_path != 0: through the folded level-0 path those kernels
 * use for the sky behind a pixel and for a ray that misses; levels is then not read and may be null.  Fails when no environment is set or
 * n == 0.  Reads the decoded cube only: no frame state, no input set and no still-sky run is touched.  Synchronises the main stream. */
int  rtggx_debug_environment(rtggx_context* ctx, const float* dirs3, const float* levels, uint32_t n, int level0_path, float* rgb3);
int  rtggx_get_timings(rtggx_context* ctx, RtggxTimings* out);
/* mode 0 off, 1 every pass (rtggx_get_timings), 2 only the ray-trace kernel: one HIP event pair per frame,
 * recorded on the launching stream right around the kernel, kept for up to RTGGX_KERNEL_RING frames; 3 like 2 for
 * every 8th frame only (an event pair costs the launching stream ~6 us per frame). */
#define RTGGX_KERNEL_RING 4096
int  rtggx_enable_timing(rtggx_context* ctx, int mode);
/* Durations (ms) of the ray-trace kernel launches recorded in mode 2 or 3 since the last call; synchronises. */
int  rtggx_kernel_times(rtggx_context* ctx, float* ms, uint32_t capacity, uint32_t* count);

/* Diagnostic: the shader clock (MHz) the device runs at while the call is in flight -- one idle wave on the refit stream compares the
 * shader-cycle counter with the 100 MHz real-time counter over ~20 us; other streams keep running.  Synchronises only that stream. */
int  rtggx_debug_shader_clock(rtggx_context* ctx, double* mhz);

/* Attainable HBM bandwidth of the device (GB/s, read + written bytes): a float4 copy kernel over two buffers of `bytes` each,
 * `iterations` timed launches for each of four launch shapes (2 / 4 / 8 / 16 workgroups per CU: the shape matters by 20 % on MI355X), the
 * best one reported.  For the measured peak bench.py quotes beside the vendor figure; synchronises. */
int  rtggx_copy_bandwidth(rtggx_context* ctx, size_t bytes, int iterations, double* gbytes_per_s);

/* Size in bytes of a buffer / synchronous copy into caller memory / raw device pointer. */
int  rtggx_buffer_size(rtggx_context* ctx, int buffer_id, size_t* bytes);
int  rtggx_readback(rtggx_context* ctx, int buffer_id, void* dst, size_t bytes);
int  rtggx_buffer_ptr(rtggx_context* ctx, int buffer_id, void** device_ptr);
/* Overwrite a render target from host memory (tests feed one pass with another implementation's input). */
int  rtggx_upload(rtggx_context* ctx, int buffer_id, const void* src, size_t bytes);
int  rtggx_frame_parity(rtggx_context* ctx, uint32_t* parity);
int  rtggx_bvh_root(rtggx_context* ctx, uint32_t slot, int32_t* root);

/* Closest-hit queries on the device for tests: rays = n x {o.xyz, d.xyz, tmin, tmax},
 * out = n x {t, instance(bits), primitive(bits), b1, b2, valid}. */
int  rtggx_trace_rays(rtggx_context* ctx, const float* rays, uint32_t n, float* out);

/* Occlusion queries: the same ray list -- rays = n x {o.xyz, d.xyz, tmin, tmax} -- through the ANY-HIT variant of the traversal
 * (csrc/trace.hip, csrc/rt_queue.h).  occluded = n words, 1 where some triangle of either instance satisfies tmin < t < tmax (both
 * bounds exclusive) under the traversal's own watertight test, 0 otherwise: by construction the `valid` of the closest-hit query on
 * the same ray.  Which triangle stopped an occluded ray is unspecified and is not reported: a lane leaves its ray at the first
 * triangle it accepts, its pending subtrees are dropped, and nothing is ordered by distance.  Like the closest-hit query it refills
 * a set's ray bins, so it waits for the frames in flight and ends the still-sky runs; the frames after it are what they would have
 * been without it.  The rays are not added to the frame's ray counters.  Fails on n == 0, on a null pointer and before
 * rtggx_build_as / the first rtggx_update_frame.  Opt-in: a context that never calls it launches no any-hit kernel. */
int  rtggx_trace_occlusion(rtggx_context* ctx, const float* rays, uint32_t n, uint32_t* occluded);

/* A sun: one directional light with ray-traced shadows.  Opt-in: a context that never calls this allocates and launches what it always did.
 * direction: a world-space vector TOWARD the sun, normalised on the host in double and rounded once to fp32 (call it L).  irradiance: E, rgb,
 * what a surface facing the sun receives, in the units of the environment's radiance x sr.  (NULL, NULL) or E = 0 in every component turns
 * the sun off.  Takes effect with the next rtggx_render_visibility.  Refused, the context keeping what it had: a non-finite or zero-length
 * direction; a negative or non-finite E; a sun on a context at ray rate 4, and rate 4 on a context with a sun (three quarters of a rate-4
 * frame are interpolations).
 * While the sun is on rtggx_ray_trace runs three more kernels behind the hit shading (and the resolve of N samples), in front of the
 * accumulation, the scoring and rtggx_denoise; RtggxTimings.ray_trace covers them.  For every covered pixel (visibility word != 0) of the
 * rows ray generation covers, in fp32 without contraction, each operation rounded on its own:
 *   1. the primary surface exactly as ray generation derives it: P, N, V, color, (r, m), inst, prim;
 *   2. NoL = dot(N, L); NoL <= 0: no ray, both words untouched;
 *   3. a shadow ray from P along L, interval (1e-5, 10000), skipping (inst, prim), through the any-hit traversal; occluded: both words untouched;
 *   4. r' = max(r, 1/32) (a mirror under a delta light has no finite answer); H = normalize(V + L); NoH, VoH, NoV saturated; a = r' r', a2 = a a;
 *      d = (NoH a2 - NoH) NoH + 1; D = a2 / ((pi d) d); f0 = lerp(0.04, color, m); F = fSchlick(f0, VoH); vis = visSmith(r', NoV, NoL);
 *      k = (D vis) NoL; spec_c = (F_c k) E_c; RayTracingOut0 = pack(unpack(RayTracingOut0) + spec);
 *   5. where m < 1: diff_c = ((color_c (1 - 0.04)) (NoL / pi)) E_c; RayTracingOut1 = pack(unpack(RayTracingOut1) + diff).  Where m >= 1
 *      RayTracingOut1 is a carry-over and is not touched.
 * The terms are added to the packed words: one more rounding of at most half a code of an 11-bit float, and the sun is independent of recursion
 * depth, sample count, sample set and sample map -- one shadow ray per covered, sun-facing pixel per frame, counted by rtggx_ray_count.
 * Background pixels are untouched.  Setting the sun ends no still-sky run and resets no accumulation (the caller's to do).
 * Known limit: surfaces seen in reflections are shaded by the environment and the SH irradiance alone -- a reflection shows the ground
 * without its sun term and without the shadow.  rtggx_set_sun_reflections(ctx, 1) lifts the limit.  Known limit: the light is a
 * direction, so every shadow edge is one pixel hard; rtggx_set_sun_angle gives the sun a size and the shadows a penumbra.  Memory: 56 bytes per pixel and 4 per
 * 8x8 block, from the first call that turns it on. */
int  rtggx_set_sun(rtggx_context* ctx, const float direction[3], const float irradiance[3]);

/* The sun at the surfaces the paths hit: every surface seen in a reflection (or by a diffuse ray), at every recursion level, gets the sun's
 * term and its shadow.  enable: 0 (the default) or 1; anything else is refused and the setting kept.  The setting is stored whether or not a
 * sun is set and does something only in frames where the sun is on (so never at ray rate 4, which the sun excludes); it takes effect with
 * the next rtggx_render_visibility.  Opt-in: a context that never asks for it allocates and launches exactly what it did.
 * A path of recursion depth D: its level-d ray (o, dir) carries the throughput T_d, T_0 = w0, T_{d+1} = T_d w_{d+1} -- the weight of the ray's
 * record, as the hit shading reads it.  The ray TOUCHES A SURFACE when it hits and is not a reflection-group ray whose preset is <= 0 in every
 * component (that one returns the preset without looking at the surface).  For such a ray, with the hit derived exactly as the hit shading
 * derives it -- triangle from the hit id, barycentrics from the repeated watertight test, N, (r, m), color, V = -dir, P = o + t dir per
 * component --, in fp32 without contraction, each operation rounded on its own:
 *   1. NoL = dot(N, L); NoL <= 0: no shadow ray, no term;
 *   2. a shadow ray from P along L, interval (1e-5, 10000), skipping the hit's (inst, prim), through the any-hit traversal; occluded: no term.
 *      rtggx_ray_count / rtggx_ray_total count it;
 *   3. the lobe the path uses at that surface.  m > 0.5: step 4 of rtggx_set_sun with this hit's N, V, (r, m), color: term_c = (F_c k) E_c.
 *      Otherwise color' = color (1 - m) for a diffuse-group ray, color for a reflection-group ray; term_c = (color'_c (NoL / pi)) E_c (no
 *      x 0.96: the rule of the hit shading at depth >= 1);
 *   4. s_d = T_d term, per component.
 * One sample per pixel: per (pixel, image the path writes) S = +0, then S = S + s_d for d ascending over the levels that have a term; behind
 * the last shading pass word = pack(unpack(word) + S) where at least one term exists, the word untouched bit for bit where none does.  N > 1
 * samples, with or without a sample map: the terms go into the pixel's fp32 sums -- sample after sample, levels ascending, at level d
 * acc = acc + s_d first and then the value of a path that ends at level d; the resolve and its 1 / c scale are unchanged, and a block that
 * has had its c samples traces no shadow ray.  No atomics: at most one live path exists per (pixel, image) and pass, and the order of every
 * sum is the order of the launches.  The pass of rtggx_set_sun still runs afterwards, unchanged, on the packed words.  Background pixels
 * get no term; where the pixel's metallic is >= 1 RayTracingOut1 gets none (no path writes it).  The rule is independent of sampler,
 * sample-set size and stream placement.
 * Per level and sample three more kernels in front of the hit shading pass (one generating the shadow rays from the level's hits, the
 * any-hit traversal, one adding the unoccluded terms), and one more behind the last pass of a one-sample frame.  Memory, from the first
 * frame that has both the sun and this on: a queue of the frame's bin size -- 56 bytes per ray slot, i.e. 56 bytes per pixel while both
 * materials are fully metallic and 112 from the first metallic below 1 -- and 4 bytes per 8x8 block; a one-sample frame adds S, 32 bytes
 * per pixel (two images of r, g, b and the number of terms).  S is all zero between frames: the pass that adds it to the words clears what it
 * found set. */
int  rtggx_set_sun_reflections(rtggx_context* ctx, int enable);

/* A sun with a size: the shadow rays of rtggx_set_sun and of rtggx_set_sun_reflections point at a point of the sun's disk instead of at its
 * centre -- a penumbra, one sample per ray and frame, which the temporal pass or rtggx_set_accumulation average.  degrees: the angular
 * RADIUS of the disk (the real sun: 0.27); 0, the default, is the directional sun.  The value is stored whether or not a sun is set and acts
 * only in frames where the sun is on; it takes effect with the next rtggx_render_visibility.  Refused, the context keeping what it had: a
 * NaN, a negative value, more than RTGGX_MAX_SUN_ANGLE_DEGREES.  The cap: the BRDF and NoL are still evaluated at the centre direction L --
 * the usual approximation for a small disk, and not a good one for a wide source.  Opt-in: a context that never calls this, or calls it with
 * 0, allocates and launches exactly what it did; no device buffer is added.  rtggx_sun_from_env does not set an angle: its cone is a policy
 * default, not a measurement of the disk.
 * Host, once per call of this function (k) or of rtggx_set_sun (T, B), in double on the stored fp32 L, each result rounded once to fp32:
 *   k = 1 - cos(degrees pi / 180);  a = the coordinate axis of the smallest |L_i|, ties to the lowest index;  T = normalize(cross(a, L));
 *   B = cross(L, T) (of the unrounded T).
 * Per shadow ray, in fp32 without contraction, each operation rounded on its own:
 *   1. h = rng(rng(pixel) + FrameIndex): the word getSampleParam forms before it masks it.  pixel: the full-frame pixel index y W + x (strips
 *      agree with the whole frame).  FrameIndex: the frame's own for the pass of rtggx_set_sun; for the hits of sample k of an N-sample
 *      frame sample k's, FrameIndex N + k;
 *   2. w = rng(h + j 0x9E3779B9), j = 0 for the pass of rtggx_set_sun and 1 + 2 d + i for the hit of a level-d ray of the path that writes
 *      image i (0: RayTracingOut0, the reflection group's; 1: RayTracingOut1, the diffuse group's);
 *   3. u = (float)(w & 0xffff) / 65536;  s = w >> 24;  cos(phi), sin(phi) = entry s of the 256-entry table of the default sample set,
 *      whatever rtggx_set_sample_set is: the sun is independent of the sample set;
 *   4. e = u k;  cos(theta) = 1 - e;  sin(theta) = sqrt(e (2 - e)), correctly rounded (not 1 - cos^2, which cancels at small angles):
 *      uniform in solid angle over the cap;
 *   5. Ls_c = ((T_c (cos(phi) sin(theta))) + (B_c (sin(phi) sin(theta)))) + L_c cos(theta), per component, not renormalised;
 *   6. a ray exists where NoL = dot(N, L) > 0, as before, AND dot(N, Ls) > 0.  Where the second test fails -- "below the horizon" -- there is
 *      no ray and no term, and rtggx_ray_count counts nothing.  Otherwise the shadow ray goes from P along Ls over (1e-5, 10000), skipping
 *      the surface's triangle;
 *   7. the term added where the ray is unoccluded is the directional sun's bit for bit: BRDF and NoL at L.  Only visibility is sampled -- a
 *      pixel lit from the whole disk carries the directional sun's word, a penumbra pixel carries it in a fraction of the frames.
 * Everything else -- the queues, the any-hit traversal, the adds, the order of the sums, the streams -- is that of the two sun passes. */
#define RTGGX_MAX_SUN_ANGLE_DEGREES 10.0f
int  rtggx_set_sun_angle(rtggx_context* ctx, float degrees);

/* Local lights: up to RTGGX_MAX_LIGHTS point and spot lights inside the scene, each with a range, an optional cone, an optional radius (an
 * emitting sphere: soft shadows) and ray-traced shadows.  Opt-in: (NULL, 0) turns the lights off, and a context that never calls this, or has
 * count == 0, allocates and launches exactly what it did.  The lights are copied before the call returns and take effect with the next
 * rtggx_render_visibility, like the sun.  With a cone the axis is normalised on the host in double and rounded once to fp32 (call it A), the
 * rule of the sun's direction.  Refused, the context keeping what it had: count > RTGGX_MAX_LIGHTS; a null pointer with count > 0; in any
 * light a non-finite position; a range that is not finite or not above 0; a non-finite or negative intensity component; a radius that is not
 * finite, is negative, or is >= the range; with cos_outer > -1 an axis that is non-finite or zero, or cosines that do not satisfy
 * -1 < cos_outer < cos_inner <= 1; lights on a context at ray rate 4, and rate 4 on a context with lights (the sun's rule, for the sun's
 * reason).  A light whose intensity is 0 in every component stays in the list and casts no ray: it keeps its index i, and so the hash slots
 * of the lights behind it.
 * While count > 0 rtggx_ray_trace runs the lights' pass on the main stream: behind the hit shading, the resolve of N samples and the sun's
 * pass where there is one; in front of the accumulation, the scoring and rtggx_denoise; RtggxTimings.ray_trace covers it.  For every covered
 * pixel (visibility word != 0) of the rows ray generation covers, in fp32 without contraction, each operation rounded on its own (sqrt and /
 * correctly rounded; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; normalize(v) = v (1 / sqrt(dot(v, v)))):
 *   0. the primary surface exactly as in step 1 of rtggx_set_sun: P, N, V, color, (r, m), inst, prim.  S0 = S1 = (+0, +0, +0), n = 0.
 * Per light i = 0 .. count - 1, ascending, whose intensity I is not 0 in every component; Pl its position, R its range, rho its radius:
 *   1. D = Pl - P per component; d2 = dot(D, D).  d2 < 1e-6 or d2 >= R R: no ray, no term ("out of range");
 *   2. L = normalize(D); NoL = dot(N, L); NoL <= 0: no ray, no term ("facing away");
 *   3. only where cos_outer > -1: c = -dot(L, A); c <= cos_outer: no ray, no term ("outside the cone");
 *      s = saturate((c - cos_outer) / (cos_inner - cos_outer)); spot = s s.  Without a cone spot = 1;
 *   4. q = d2 / (R R); win = saturate(1 - q q), then win = win win; m2 = max(rho rho, 1e-4); att = (win spot) / max(d2, m2); E_c = I_c att;
 *   5. the target.  rho = 0: Ds = D.  rho > 0: h = rng(rng(pixel) + FrameIndex) -- pixel: the full-frame index y W + x (strips agree with
 *      the whole frame); FrameIndex: the constants' own, whatever N, the map or the sample set are --; w = rng(h + (16 + i) 0x9E3779B9) with
 *      32-bit wraparound (the sun's passes use the slots 0 .. 8; the lights start at 16); u = (float)(w & 0xffff) / 65536; s = w >> 24;
 *      cos(phi), sin(phi) = entry s of the 256-entry table of the default sample set, as in step 3 of rtggx_set_sun_angle; z = 1 - 2 u
 *      (exact); rho' = sqrt(1 - z z); o = (rho' cos(phi), rho' sin(phi), z), uniform on the sphere; Ds_c = D_c + rho o_c.  In both cases
 *      ds2 = dot(Ds, Ds); ds2 < 1e-6: no ray, no term; Ls = normalize(Ds); tmax = sqrt(ds2).  With rho = 0 Ls and L are the same bits;
 *   6. dot(N, Ls) <= 0: no ray, no term ("below the horizon"; with rho = 0 it cannot differ from step 2);
 *   7. a shadow ray from P along Ls over (1e-5, tmax), both bounds exclusive, skipping (inst, prim), through the any-hit traversal: the light
 *      is not geometry, and nothing behind the target occludes.  rtggx_ray_count / rtggx_ray_total count it.  Occluded: no term;
 *   8. the term, as in step 4 of rtggx_set_sun with this L and E, evaluated at the centre direction L (only visibility is sampled, as with
 *      the sun's disk): r' = max(r, 1/32); H, NoH, VoH, NoV, D, f0, F, vis as there; k = (D vis) NoL; spec_c = (F_c k) E_c; S0 = S0 + spec.
 *      Where m < 1: g = (NoL / pi) att; diff_c = ((color_c (1 - 0.04)) g) I_c; S1 = S1 + diff.  n = n + 1.
 * Behind the last light, where n > 0: RayTracingOut0 = pack(unpack(RayTracingOut0) + S0), and where also m < 1 RayTracingOut1 =
 * pack(unpack(RayTracingOut1) + S1).  Where n = 0 both words stay bit for bit; where m >= 1 RayTracingOut1 is a carry-over and is never
 * touched; background pixels are untouched.  The order of every sum is the order of the lights; there are no atomics, and the image is a pure
 * function of the inputs.  The pass is independent of recursion depth, sample count, sample map, sample set and sampler; it ends no still-sky
 * run and resets no accumulation; it works on strips, with a deforming mesh, a caller-owned stream and rtggx_set_async_compute(0).
 * Known limit: surfaces seen in reflections get no light term -- a reflection shows the ground without the lamp and without its shadow.
 * rtggx_set_light_reflections(ctx, 1) lifts the limit.
 * Per light three kernels (one generating the shadow rays, the any-hit traversal, one adding the unoccluded terms to S), and one more behind
 * the last light.  Memory, from the first frame with lights until rtggx_destroy: ONE queue for all lights with the rays' intervals beside it --
 * 56 + 8 bytes per pixel and 4 per 8x8 block -- and S, 32 bytes per pixel (two images of r, g, b and the number of terms), all zero between
 * frames.  tests/lights_ref.cpp restates the rule. */
typedef struct RtggxLight {                 /* 64 bytes */
  float position[3];  float range;          /* world space; R > 0: at and beyond R the light does nothing */
  float intensity[3]; float radius;         /* I, rgb: radiant intensity, E = I / d^2 in the units of rtggx_set_sun's E; rho >= 0: radius of the emitting sphere */
  float axis[3];      float cos_outer;      /* spot: axis points FROM the light INTO the scene; cos_outer <= -1: no cone (a point light), axis not read */
  float cos_inner;    float pad[3];         /* pad is not read */
} RtggxLight;
#define RTGGX_MAX_LIGHTS 8u
int  rtggx_set_lights(rtggx_context* ctx, const RtggxLight* lights, uint32_t count);

/* The lights at the surfaces the paths hit: every surface seen in a reflection (or by a diffuse ray), at every recursion level, gets the
 * lights' terms and their shadows -- the counterpart of rtggx_set_sun_reflections.  enable: 0 (the default) or 1; anything else is refused and
 * the setting kept.  The setting is stored whether or not lights are set and acts only in frames that have count > 0 lights (so never at ray
 * rate 4, which lights exclude); it takes effect with the next rtggx_render_visibility.  Opt-in: a context that never enables it, or has no
 * lights, allocates and launches exactly what it did.
 * A level-d ray (o, dir) of a path carries the throughput T_d as in rtggx_set_sun_reflections, and TOUCHES A SURFACE under that function's
 * definition: it hits, and it is not a reflection-group ray whose preset is <= 0 in every component.  For such a ray the hit is derived exactly
 * as the hit shading and rtggx_set_sun_reflections derive it -- triangle from the hit id, barycentrics from the repeated watertight test, N,
 * (r, m) and color of the hit's instance, V = -dir, P = o + t dir per component.  Then per light i = 0 .. count - 1, ascending, whose intensity
 * I is not 0 in every component, in fp32 without contraction, each operation rounded on its own, with the operator definitions of
 * rtggx_set_lights:
 *   1. steps 1-4 of rtggx_set_lights with this P and N: out of range (d2 < 1e-6 or d2 >= R R), facing away (NoL <= 0), outside the cone
 *      (c <= cos_outer) -- each: no ray, no term --; spot; att = (win spot) / max(d2, m2);
 *   2. step 5, the target Ds, with h = rng(rng(pixel) + F) and w = rng(h + j 0x9E3779B9).  pixel: the path's pixel as a full-frame index
 *      y W + x.  F: the frame's FrameIndex at one sample; for sample k of an N-sample frame FrameIndex N + k, the sun hits' rule.
 *      j = 32 + 16 d + 8 img + i, img the image the path writes (0: RayTracingOut0, 1: RayTracingOut1): the sun's passes use the slots 0 .. 8
 *      and the primary lights 16 .. 23, so 32 .. 95 collide with neither.  u, s, z, rho', o and Ds_c = D_c + rho o_c as there; ds2 < 1e-6: no
 *      ray, no term.  With rho = 0 there is no hash, and Ls and L are the same bits;
 *   3. steps 6-7: dot(N, Ls) <= 0: no ray, no term ("below the horizon"); else a shadow ray from P along Ls over (1e-5, tmax), tmax =
 *      sqrt(ds2), both bounds exclusive, skipping the hit's (inst, prim), through the any-hit traversal.  rtggx_ray_count / rtggx_ray_total
 *      count it.  Occluded: no term;
 *   4. the term of the lobe the path uses at that surface (step 3 of rtggx_set_sun_reflections), at the centre direction L.  m > 0.5:
 *      r' = max(r, 1/32); H, NoH, VoH, NoV, D, f0, F, vis and k = (D vis) NoL as in step 8 of rtggx_set_lights; term_c = (F_c k) (I_c att).
 *      Otherwise color' = color (1 - m) for a diffuse-group ray, color for a reflection-group ray; g = (NoL / pi) att; term_c = (color'_c g) I_c
 *      (no x 0.96: the rule of the hit shading at depth >= 1);
 *   5. s = T_d term, per component.
 * The sums.  There is ONE S per (pixel, image); where rtggx_set_sun_reflections is active as well the two features share it.  One sample per
 * pixel: S = +0; for d ascending first the sun's s_d (where that feature is active and has a term), then the lights' terms for i ascending;
 * behind the last shading pass word = pack(unpack(word) + S) where at least one term of either feature exists, the word untouched bit for bit
 * where none does -- one rounding whichever features are on.  N > 1 samples, with or without a sample map: the terms go into the pixel's fp32
 * sample sums in the same order -- sun, then lights ascending --, at each level in front of the value of a path that ends there; the resolve
 * and its 1 / c scale are unchanged, and a block that has had its c samples traces no shadow ray.  The primary passes of rtggx_set_sun and
 * rtggx_set_lights still run afterwards, unchanged, on the packed words.  Background pixels get no term; where the pixel's metallic is >= 1
 * RayTracingOut1 gets none.  No atomics; the image is a pure function of the inputs, independent of sampler, sample-set size and stream
 * placement.
 * Per light with an intensity, level and sample three more kernels in front of the hit shading pass (one generating the shadow rays from the
 * level's hits, the any-hit traversal in the frame's launch shape, one adding the unoccluded terms), and one more behind the last pass of a
 * one-sample frame unless the sun's hit pass already runs it: the cost grows with lights x levels x samples and is not shaped by the number
 * of shadow rays (DESIGN.md section 9 "The lights in reflections" has the measurements).  Memory, from the first frame that has lights and
 * this on: a queue of the frame's bin size with the rays' intervals beside it -- 56 + 8 + 8 bytes per ray slot -- and 4 bytes per 8x8 block;
 * a one-sample frame adds S, 32 bytes per pixel, unless rtggx_set_sun_reflections already allocated it.  S is all zero between frames.
 * tests/light_hit_ref.cpp restates the rule. */
int  rtggx_set_light_reflections(rtggx_context* ctx, int enable);

/* One shadow ray per surface point for ALL local lights: the pass picks one light per point, in proportion to the luminance that light would
 * contribute unshadowed, traces its one shadow ray and divides the term by the probability of the pick.  The expectation over the draw is
 * the sum rtggx_set_lights computes; the cost is noise where lights of different visibility overlap, which the temporal pass and
 * rtggx_set_accumulation average as they average penumbrae.
 * mode 0 (default): every light traces its own shadow ray (rtggx_set_lights as it is).
 * mode 1: one shadow ray per surface point for all lights.
 * Any other mode is refused and the setting kept.  The mode is stored whether or not lights are set and acts only in frames that have
 * count > 0 lights (so never at ray rate 4, which lights exclude); it takes effect with the next rtggx_render_visibility.  Opt-in: a context
 * in mode 0 allocates and launches exactly what it did.  RTGGX_MAX_LIGHTS and rtggx_set_lights with its refusals are unchanged.
 * The primary pass in mode 1, in place of the per-light steps of rtggx_set_lights; per covered pixel of the rows ray generation covers, in
 * fp32 without contraction, each operation rounded on its own, with the operator definitions of rtggx_set_lights:
 *   0. the primary surface, as in step 0 of rtggx_set_lights;
 *   1. the candidates.  For the lights in ascending index i, skipping any whose intensity is 0 in every component: steps 1-4 of
 *      rtggx_set_lights -- a light that is out of range, facing away or outside the cone is not a candidate.  spec_i is step 8 as computed
 *      there: spec_i,c = (F_c k) (I_c att).  Where m < 1: diff_i,c = ((color_c (1 - 0.04)) g) I_c with g = (NoL / pi) att.
 *      Y(c) = (0.25 c.r + 0.5 c.g) + 0.25 c.b.  w_i = Y(spec_i) + Y(diff_i); where m >= 1 w_i = Y(spec_i) alone.  A light is a candidate
 *      iff w_i > 0 (a NaN is not a candidate);
 *   2. W = ((+0 + w_a) + w_b) + ... over the candidates, ascending.  With no candidate there is no ray, and both words stay bit for bit;
 *   3. the draw.  h = rng(rng(pixel) + FrameIndex) as in step 5 of rtggx_set_lights; v = rng(h + 96 * 0x9E3779B9) with 32-bit wraparound
 *      (slot 96 is free: the sun uses the slots 0 .. 8, the primary lights 16 .. 23, the hits 32 .. 95); x = (float)(v >> 8) / 16777216,
 *      which is exact; t = x W;
 *   4. the pick.  c = +0; over the candidates, ascending, c = c + w_i; the chosen light is the first with t < c; if none qualifies, the last
 *      candidate;
 *   5. f = W / w_i, correctly rounded.  With a single candidate f is exactly 1;
 *   6. steps 5-7 of rtggx_set_lights for the chosen light alone, with its own slot 16 + i: the target Ds; ds2 < 1e-6, or below the horizon:
 *      no ray, no term; the shadow ray over (1e-5, tmax), skipping (inst, prim), through the any-hit traversal.  rtggx_ray_count /
 *      rtggx_ray_total count it.  Occluded: no term;
 *   7. where the ray is unoccluded: S0_c = spec_i,c f, one more multiplication; where m < 1 S1_c = diff_i,c f; n = 1; and the words are
 *      written as they are behind the last light of rtggx_set_lights: pack(unpack(word) + S), one rounding.
 * Everything else of rtggx_set_lights holds: background pixels are untouched, RayTracingOut1 at m >= 1 is a carry-over and is never touched,
 * the pass is independent of recursion depth, sample count, sample map, sample set and sampler, and it works on strips (pixel is the
 * full-frame index), with a deforming mesh, a caller-owned stream and rtggx_set_async_compute(0).  With one casting light the two images
 * are those of mode 0 bit for bit.
 * The hits in mode 1, under rtggx_set_light_reflections(ctx, 1), in place of that function's per-light steps; per level d, sample and
 * level-d ray that touches a surface, the hit derived as there: the candidates from its step 1; term_i from its step 4 and s_i = T_d term_i
 * per component; w_i = Y(s_i), a candidate iff w_i > 0; W, t, the pick and f as above, with the draw v = rng(h + (104 + 2 d + img) *
 * 0x9E3779B9), h from the path's pixel and the sample's frame index (FrameIndex N + k) -- the slots 104 .. 111 --; the chosen light's target
 * from its own slot 32 + 16 d + 8 img + i; the term added is s_i f.  The order of a pixel's sum becomes: the sun's s_d first, then this one
 * term, level by level; the sample sums, the resolve and its 1 / c scale are unchanged.
 * Per frame three kernels in place of three per light (one generating the shadow rays, the any-hit traversal, one adding the unoccluded
 * terms), and per level and sample of the hits likewise three, whatever the number of lights.  Memory in mode 1, on top of rtggx_set_lights',
 * from the first mode-1 frame with lights until rtggx_destroy: the finished diffuse term beside the lights' queue, 16 bytes per ray slot
 * (per pixel).  Known limits: the BRDF and NoL are still evaluated at the centre direction; the pick ignores visibility, so a light that is
 * mostly occluded still draws its share of rays.  tests/light_pick_ref.cpp restates the rule. */
int  rtggx_set_light_sampling(rtggx_context* ctx, int mode);

/* The pick of mode 1 weighted by what the pixel remembers: one visibility estimate per light per pixel, carried from frame to frame along the
 * velocity buffer, updated with the outcome of the one shadow ray the pixel traces anyway, and multiplied into each light's pick weight, above
 * a floor.  Every candidate keeps a non-zero probability and the term is divided by that probability: the expectation is the sum of mode 0
 * whatever the history holds, stale or wrong -- a bad reprojection costs variance, never bias.  One more 16-byte load and store per pixel, no
 * new ray and no new launch.
 * enable 0 (default) / 1; anything else is refused and the setting kept.  The setting is stored always.  It acts only in frames that run the
 * primary pass of mode 1 (rtggx_set_light_sampling(ctx, 1)) with at least one casting light -- an acting frame --, and takes effect with the
 * next rtggx_render_visibility.  The hit passes under rtggx_set_light_reflections keep mode 1's rule unchanged.  Opt-in: a context that never
 * enables it allocates and launches exactly what it did.  Whole frames only, because a reprojected tap may lie in another rank's rows:
 * enabling on a context with a strip is refused, and so is rtggx_set_strip with a strip on an enabled context.  The first acting frame
 * allocates two images of W x H records (RtggxLightVisRecord, 16 bytes), zeroed, released by rtggx_destroy.
 * The sequence.  s counts the acting frames of the context and starts at 0; an acting frame first does s = s + 1.  s0 is the value of s at
 * the last reset; resets are: the allocation, every successful rtggx_set_lights, every successful rtggx_set_light_sampling, and every change
 * of this setting.  The frame writes image s & 1 and reads image (s - 1) & 1.  Behaviour after s passes 2^24 is not specified.
 * Per covered pixel (x, y) of the pass, in fp32 without contraction, each operation rounded on its own, with the operator definitions of
 * rtggx_set_lights:
 *   1. step 0 and the candidates w_i exactly as in step 1 of mode 1's primary pass;
 *   2. the history.  (vx, vy) are the two halves of the frame's own RTGGX_BUF_VELOCITY word (binary16, vx the low one); qx = floor(((float)x + 0.5f) - vx (float)W),
 *      qy likewise with H.  R is the record at (qx, qy) of the image read.  The history is valid iff s - 1 > s0; 0 <= qx < W and
 *      0 <= qy < H; R.stamp >> 8 == (s - 1) & 0xFFFFFF; (R.stamp & 0xFF) == inst + 1; and dot(n(R.normal), n(this pixel's normal word)) >=
 *      0.9f, where n() is the decode the spatial filters use: n(word)_k = (float)(2 q_k - 1023) / 1023 of the word's three 10-bit fields --
 *      evaluated as I >= 0.9f * 1046529.0f (the constant rounded once) with I the dot of the integers 2 q_k - 1023, which is exact.  If
 *      valid v_i = R.v[i]; otherwise v_i = 255 for every i;
 *   3. the weights.  u_i = w_i (float)max(v_i, RTGGX_LIGHT_VIS_FLOOR) for the candidates; a light that is not a candidate has no weight.
 *      U = ((+0 + u_a) + u_b) + ..., ascending.  With no candidate there is no ray and no term.  The record is written in every case: the
 *      carried v, this pixel's normal word, and stamp = (s & 0xFFFFFF) << 8 | (inst + 1);
 *   4. draw, pick and f are mode 1's steps 3-5 with u in place of w and U in place of W: the same slot 96, the same "first candidate with
 *      t < c, else the last", and f = U / u_i.  With a single candidate f is exactly 1;
 *   5. target, ray and term are mode 1's steps 6-7 unchanged: S0 = spec_i f, S1 = diff_i f;
 *   6. the update, only where a shadow ray was traced ("no ray" -- below the horizon, ds2 < 1e-6 -- leaves v as carried).  For the chosen
 *      light, in integers: unoccluded v' = v + ((255 - v + 3) >> 2); occluded v' = v - ((v + 3) >> 2).  0 and 255 are reached exactly and
 *      are fixed points.  The other seven bytes keep the carried value.
 * Pixels that are not covered write nothing, and neither do waves that leave on a zero tile word; the stamp is what keeps their old records
 * from being read as history.  There are no atomics: a pixel writes only its own record and reads only the other image; the two images and
 * both traced images are a pure function of the frame sequence.
 * Known limits: the hits are not covered (a path's hit has no velocity to follow); the floor means a light that leaves shadow is noticed
 * only at 1/16 of its share; the estimates are per pixel and not filtered over neighbours.  tests/light_vis_ref.cpp restates the rule.
 * It does not act on a light list (rtggx_set_light_list): a record has eight bytes, a list up to 1024 lights --
 * rtggx_set_light_list_visibility is the list's own, with a sparse record. */
#define RTGGX_LIGHT_VIS_FLOOR 16u      /* policy default, not a measurement */
typedef struct RtggxLightVisRecord {   /* 16 bytes */
  uint8_t  v[8];      /* v[i]: visibility estimate of light i, 0 .. 255 */
  uint32_t normal;    /* the frame's RTGGX_BUF_NORMAL word of the pixel */
  uint32_t stamp;     /* (s & 0xFFFFFF) << 8 | (inst + 1); 0: never written */
} RtggxLightVisRecord;
int  rtggx_set_light_pick_visibility(rtggx_context* ctx, int enable);   /* 0 (default) / 1; anything else refused, setting kept */
/* Synchronises and copies image 0 or 1 of the records (W x H, row by row) to out; *sequence (may be NULL) receives the context's s.  It fails
 * before anything is allocated (before the first acting frame), for an image other than 0 or 1, and when bytes is not W H 16. */
int  rtggx_read_light_visibility(rtggx_context* ctx, uint32_t image /* 0, 1 */, RtggxLightVisRecord* out, size_t bytes, uint32_t* sequence);

/* Local lights beyond eight: a list of up to RTGGX_MAX_LIGHT_LIST lights in device memory, one shadow ray per surface point for all of them,
 * and per 8x8 block only the lights whose range reaches the block are looked at.  The same RtggxLight, checked as rtggx_set_lights checks it,
 * with the same refusals: a null pointer with count > 0; in any light a non-finite position; a range that is not finite or not above 0; a
 * non-finite or negative intensity component; a radius that is not finite, is negative, or is >= the range; with cos_outer > -1 an axis that
 * is non-finite or zero, or cosines that do not satisfy -1 < cos_outer < cos_inner <= 1; a list on a context at ray rate 4, and rate 4 on a
 * context with a list.  The axis is normalised in double and rounded once.  Refused as well: count > RTGGX_MAX_LIGHT_LIST; count > 0 while
 * rtggx_set_lights holds count > 0, and rtggx_set_lights with count > 0 while a list is held -- the context holds one or the other.  A
 * refused call leaves what the context had.  The list is copied before the call returns and takes effect with the next
 * rtggx_render_visibility, which uploads it; (NULL, 0) clears the list.  Opt-in: a context that never calls this, or has cleared the list,
 * allocates and launches exactly what it did.  A light whose intensity is 0 in every component stays in the list, keeps its index and casts
 * no ray.
 * The rule with a list of n lights is mode 1's rule, whatever rtggx_set_light_sampling says.  The primary pass, and under
 * rtggx_set_light_reflections(ctx, 1) the hit passes, are rtggx_set_light_sampling's steps 0-7 and its hit rule, word for word, with i
 * running 0 .. n - 1: the candidates, w_i, W summed ascending, the draw from slot 96 (the hits: 104 + 2 d + img), "the first candidate with
 * t < c, else the last", f = W / w_i, the chosen light's target, ray and term.  The only new number is the hash slot of the target of a
 * light i >= 8; below 8 the slots of rtggx_set_lights hold:
 *   primary: 16 + i for i < 8, 4096 + i for i >= 8;
 *   hits:    32 + 16 d + 8 img + i for i < 8, 8192 + 1024 (2 d + img) + i for i >= 8 (with d <= 3 it meets nothing in use).
 * The sums, the resolve, the order (the sun first, then this one term, level by level), the queue formats, strips (pixel is the full-frame
 * index), deforming meshes, caller-owned streams and rtggx_set_async_compute(0) are mode 1's.  With n <= 8 the images and the ray count
 * are those of the same lights through rtggx_set_lights in mode 1.  rtggx_set_light_pick_visibility does not act on a list: its records
 * have eight bytes; rtggx_set_light_list_visibility, further down, does.
 * The cull.  Per 8x8 block of the primary pass, over the block's covered pixels in the pass's rows: lo_c / hi_c are the fp32 minimum /
 * maximum of P_c, the P of step 0.  Per light k that casts rays (an intensity component is not 0), in fp32 without contraction, each
 * operation rounded on its own:
 *   e_c = max(max(lo_c - Pl_c, Pl_c - hi_c), 0);  dist2 = (e_x e_x + e_y e_y) + e_z e_z;  RRm = (R R) 1.000244140625f (that is 1 + 2^-12);
 *   light k is KEPT iff dist2 < RRm.
 * A light without intensity is never kept.  Lanes evaluate kept lights only.  At the hits the box is taken over the lanes of one 64-slot
 * round of a bin that hold a touched hit, from P = o + t dir.
 * The cull is invisible: for P in the box every |Pl_c - P_c| >= e_c exactly, each quantity a single rounding of an exact difference, and
 * rounding is monotonic; squares and sums of non-negative terms carry at most (1 + 2^-24)^k with k <= 8; so d2 < R R at any pixel implies
 * dist2 < R R (1 + 2^-20) < RRm.  A light that is not kept is out of range at every point of the block: its w_i is +0 there, which leaves
 * W and c as they are, and it cannot be chosen.  The images and the ray count are those of the walk over all n lights, bit for bit
 * (DESIGN.md section 9 "A culled light list"; tests/light_list_ref.cpp restates the rule without a cull and asserts the implication).
 * Per frame one generating launch, one any-hit traversal and one add, and per level and sample of the hits likewise, whatever n.  Memory: 80
 * bytes per light, mode 1's queue, sums and diffuse terms, and 4 bytes per 8x8 block for the counts below.
 * Known limits: no culling by cone or by facing; no world-space grid for the hits, whose points are incoherent (a round's box can be large:
 * the cull there saves less); visibility records at the primary pass only (rtggx_set_light_list_visibility); no more than 1024 lights; the count of a list is fixed
 * (rtggx_update_light_list moves its lights, not their number). */
#define RTGGX_MAX_LIGHT_LIST 1024u
int  rtggx_set_light_list(rtggx_context* ctx, const RtggxLight* lights, uint32_t count);
/* Synchronises and copies, row-major by 8x8 block, the number of kept lights of the last frame's primary pass: ceil(H/8) rows of ceil(W/8)
 * words.  A block with no covered pixel, or in a 16x16 tile in which nothing is drawn, reads 0 (and so does every block under a list
 * without a casting light).  Whole frames only: it fails on a context with a strip; it fails before the first frame with a list, and
 * when bytes != ceil(H/8) ceil(W/8) 4. */
int  rtggx_read_light_list_counts(rtggx_context* ctx, uint32_t* out, size_t bytes);
/* 1 (default): the cull.  0: every casting light is kept in every block that has a covered pixel (the hits: a touched hit) -- the same
 * images and ray counts, the counts equal to the number of casting lights, the time of a walk over all lights.  Anything else is refused. */
int  rtggx_debug_light_list_cull(rtggx_context* ctx, int enable);   /* 1 (default) / 0: keep every casting light */

/* A list's pick weighted by what the pixel remembers: rtggx_set_light_pick_visibility for a light list.  A record cannot hold a value per
 * light of a list of 1024, so it is sparse: the few lights the pixel has learned are hidden, four entries, and nothing for the rest -- a
 * light without an entry is believed visible.  Every candidate keeps a non-zero probability and the term is divided by that probability: the
 * expectation is the list's own sum whatever the history holds, stale, wrong or arbitrary bytes -- a bad record costs variance, never bias.
 * One more 16-byte load and store per pixel, no new ray and no new launch.
 * enable 0 (default) / 1; anything else is refused and the setting kept.  The setting is stored always.  It acts only in frames whose primary
 * pass runs a list (rtggx_set_light_list) with at least one casting light -- an acting frame --, and takes effect with the next
 * rtggx_render_visibility.  The hit passes under rtggx_set_light_reflections keep the list's rule unchanged.  rtggx_set_lights (modes 0 and
 * 1) and rtggx_set_light_pick_visibility are untouched: this setting does not act on them, nor that one on a list.  Opt-in: a context that
 * never enables it allocates and launches exactly what it did.  Whole frames only, because a reprojected tap may lie in another rank's rows:
 * enabling on a context with a strip is refused, and so is rtggx_set_strip with a strip on an enabled context.  The first acting frame
 * allocates two images of W x H records (RtggxLightListVisRecord, 16 bytes), zeroed, released by rtggx_destroy.
 * The sequence.  s counts this setting's acting frames and starts at 0 (it is not rtggx_set_light_pick_visibility's s); an acting frame
 * first does s = s + 1.  s0 is the value of s at the last reset; resets are: the allocation, every successful rtggx_set_light_list, and every
 * change of this setting.  The frame writes image s & 1 and reads image (s - 1) & 1.  Behaviour after s passes 2^24 is not specified.
 * An entry is 16 bits: (v << 10) | light with v in 0 .. 62 and light in 0 .. 1023; 0xFFFF is a free entry (v = 63 is never stored by the
 * update: a light that reaches 63 leaves the record).  An entry other than 0xFFFF whose v field reads 63 -- arbitrary bytes can hold one --
 * is an entry like any other.
 * Per covered pixel (x, y) of the primary pass, in fp32 without contraction, each operation rounded on its own, with the operator definitions
 * of rtggx_set_lights:
 *   1. step 0 and the candidates w_i exactly as the list's primary pass has them (rtggx_set_light_sampling's steps 0-1 with i running over
 *      the list);
 *   2. the history, word for word step 2 of rtggx_set_light_pick_visibility: qx = floor(((float)x + 0.5f) - vx (float)W), qy likewise with H,
 *      from the frame's own RTGGX_BUF_VELOCITY word; R is the record at (qx, qy) of the image read.  The history is valid iff s - 1 > s0;
 *      0 <= qx < W and 0 <= qy < H; R.stamp >> 8 == (s - 1) & 0xFFFFFF; (R.stamp & 0xFF) == inst + 1; and I >= 0.9f * 1046529.0f with I the
 *      integer dot of the two normal words' 2 q_k - 1023.  If valid the four entries are R's; otherwise all four are free;
 *   3. the weights.  v_i is the v of the entry, not free, whose light field equals i -- the one of lowest index k, should two name the same
 *      light, which the update never produces -- and 63 where there is none.  u_i = w_i (float)max(v_i, RTGGX_LIGHT_LIST_VIS_FLOOR) for the
 *      candidates.  U = ((+0 + u_a) + u_b) + ..., ascending.  The record is written in every case, whether or not there is a candidate: the
 *      carried entries, this pixel's normal word, and stamp = (s & 0xFFFFFF) << 8 | (inst + 1).  With no candidate there is no ray and no term;
 *   4. draw, pick and f are the list's with u in place of w and U in place of W: slot 96, "the first candidate with t < c, else the last",
 *      f = U / u_i.  With a single candidate f is exactly 1;
 *   5. target, ray and term are the list's, unchanged, with the list's hash slots: S0 = spec_i f, S1 = diff_i f;
 *   6. the update, only where a shadow ray was traced ("no ray" -- below the horizon, ds2 < 1e-6 -- leaves the entries as carried).  For the
 *      chosen light i, in integers: k is the slot whose entry, not free, holds i (the lowest such k); v is that entry's, or 63 if there is no
 *      such slot.  unoccluded v' = v + ((63 - v + 3) >> 2); occluded v' = v - ((v + 3) >> 2).  0 and 63 are reached exactly and are fixed
 *      points.  If the slot exists it becomes 0xFFFF when v' == 63, else (v' << 10) | i.  If no slot exists and the ray is occluded (v' =
 *      47), the entry (47 << 10) | i is inserted: into the free slot of lowest k; with no free slot, in place of the entry of greatest v,
 *      ties to the lowest k.  If no slot exists and the ray is unoccluded nothing changes.  The other slots keep the carried value.
 * Pixels that are not covered write nothing, and neither do waves that leave on a zero tile word; the stamp keeps their old records from
 * being read as history.  There are no atomics: a pixel writes only its own record and reads only the other image; records and images are a
 * pure function of the frame sequence.  The cull stays invisible: a light that is not kept has w_i = +0 and is no candidate, its entry, if
 * any, is simply carried; images, ray counts AND records are those of the walk over all lights, bit for bit, with
 * rtggx_debug_light_list_cull(ctx, 0) as with the cull on.  With one casting light the images are the list's own.
 * Known limits: the hits are not covered; four entries per pixel -- a fifth hidden light evicts the least hidden; the floor means a light
 * that leaves shadow is noticed at 1/16 of its share; records are per pixel and not filtered over neighbours; strips are refused; a light
 * that moves (rtggx_update_light_list) keeps its entries, stale as they may be, until the outcomes of new rays correct them -- unbiased,
 * variance only.  tests/light_list_vis_ref.cpp restates the rule over all lights. */
#define RTGGX_LIGHT_LIST_VIS_ENTRIES 4u
#define RTGGX_LIGHT_LIST_VIS_FLOOR   4u      /* policy default, not a measurement: 1/16 of 63, as RTGGX_LIGHT_VIS_FLOOR is of 255 */
typedef struct RtggxLightListVisRecord {     /* 16 bytes */
  uint16_t entry[4];   /* (v << 10) | light: v 0..62, light 0..1023; 0xFFFF: free */
  uint32_t normal;     /* the frame's RTGGX_BUF_NORMAL word of the pixel */
  uint32_t stamp;      /* (s & 0xFFFFFF) << 8 | (inst + 1); 0: never written */
} RtggxLightListVisRecord;
int  rtggx_set_light_list_visibility(rtggx_context* ctx, int enable);      /* 0 (default) / 1; anything else refused, setting kept */
/* Synchronises and copies image 0 or 1 of the records (W x H, row by row) to out; *sequence (may be NULL) receives this setting's s.  It
 * fails before anything is allocated (before the first acting frame), for an image other than 0 or 1, and when bytes is not W H 16. */
int  rtggx_read_light_list_visibility(rtggx_context* ctx, uint32_t image /* 0, 1 */, RtggxLightListVisRecord* out, size_t bytes, uint32_t* sequence);

/* Lights of a list that move: per-frame updates without a drain, the records kept.  rtggx_set_light_list stays the way to give a context
 * a NEW list -- its next rtggx_render_visibility waits for every stream and resets the records' history --; the two calls below replace
 * lights first .. first + count - 1 of the list the context holds: the list that will be in effect at the next rtggx_render_visibility,
 * including one set by a rtggx_set_light_list that has not taken effect yet.  The number of lights never changes: indices keep their
 * meaning, and with it the hash slots and the light field of the sparse records.  Calls apply in call order and take effect with the next
 * rtggx_render_visibility.  Refused, everything staying as it was: no list held; first + count above the list's count; a null pointer with
 * count > 0.  count == 0 succeeds and does nothing.  Neither call waits for the GPU in the steady state (the first update of a context's
 * life allocates: a ring of eight versions of the list, 80 bytes per light of RTGGX_MAX_LIGHT_LIST each, and as much pinned memory);
 * neither ends a still-sky run, resets an accumulation or resets rtggx_set_light_list_visibility's history: s0 stays.  Once an update has
 * taken effect the frame's images, ray count, kept counts and records are exactly those of the list's rule above applied to the updated
 * list: the cull, the pick, the slots and the records' update are untouched, only WHICH list a frame reads is new.  Frames already in
 * flight keep reading the list they started with: a version of the list is written once, read by every frame until the next update takes
 * effect, and written again only when the last frame that read it has ended.  A frame without an update launches and copies nothing
 * beyond what it did.  Opt-in: a context that never calls these allocates and launches exactly what it did.
 * rtggx_update_light_list (a host array): every light is checked exactly as rtggx_set_light_list checks it, a cone's axis normalised in
 * double and rounded once; one invalid light refuses the whole call.  The lights are copied before the call returns; they reach the device
 * through pinned memory and an asynchronous copy on the stream of the next frame's visibility pass.  The list's kernel variant (cone,
 * radius) and whether it casts at all are recomputed from what the host knows.
 * rtggx_update_light_list_device (a device pointer, aligned to 16 bytes): ordered like hipMemcpyAsync on hip_stream (NULL means the null
 * stream), as rtggx_refit_as_device is: the read of device_lights is ordered behind what the stream holds at the call, and what the caller
 * enqueues there afterwards is ordered behind the read.  No host copy and no wait.  The host cannot see the values, so a kernel on the
 * device applies the same checks per light.  An invalid light is a REJECT: any refusal reason above, and a radius > 0 or a cone
 * (cos_outer > -1) whose kind is not declared in `kinds` (RTGGX_LIGHT_KIND_RADIUS | RTGGX_LIGHT_KIND_CONE; anything else is refused).  A
 * reject becomes a light that casts nothing -- position 0, range 1, intensity 0, no radius, no cone, cull radius 0 --, is never kept and
 * never evaluated, keeps its index, and is counted in a 64-bit counter on the device.  `kinds` is ORed into the list's variant and never
 * shrinks until the next rtggx_set_light_list; the variants are bit-identical in what they compute (a point light runs the cone variant
 * with the neutral cone (-2, -1)): a matter of speed only.
 * The one place where the semantics differ from a host-known list: from the first device update until the next rtggx_set_light_list the
 * list is PRESUMED CASTING.  The frame launches the list's three kernels, and with rtggx_set_light_list_visibility(ctx, 1) it is an
 * acting frame (s advances, records are written), whether or not any light has an intensity.  If a rtggx_set_light_list is still pending
 * when the device call comes, that list is uploaded then and there (through the staging; the call may wait as a set-up step does).
 * A host update of lights that a device update wrote, and the reverse, apply in call order.
 * rtggx_read_light_list synchronises and returns the list the last frame read, as the kernels see it: 64 bytes per light in RtggxLight's
 * layout, axis normalised (zero where there is no cone), the neutral cone (-2, -1) where there is none, pad 0, rejects in their sanitised
 * form.  It fails before the first frame with a list, and when bytes != count 64.
 * rtggx_read_light_list_rejects synchronises (the streams the device updates were given included) and returns the number of rejects since
 * the last reset; reset 1 clears it.
 * rtggx_debug_visibility_drains: how often rtggx_render_visibility has waited for every stream of the context since the last reset (a host
 * counter, one increment per wait): a rtggx_set_light_list that takes effect is one, an update is none.
 * Known limits: the count is fixed; a moved light keeps its stale record entries until the outcomes of new rays correct them -- unbiased,
 * variance only; a device-updated list is presumed casting; the frame that takes an update records one more event on the main stream.
 * DESIGN.md section 9 "Moving light lists"; tests/light_list_moving_ref.py restates the semantics on the records' restatement. */
#define RTGGX_LIGHT_KIND_RADIUS 1u   /* some light has radius > 0 */
#define RTGGX_LIGHT_KIND_CONE   2u   /* some light has cos_outer > -1 */
int  rtggx_update_light_list(rtggx_context* ctx, const RtggxLight* lights, uint32_t first, uint32_t count);
int  rtggx_update_light_list_device(rtggx_context* ctx, const RtggxLight* device_lights, uint32_t first, uint32_t count, uint32_t kinds, void* hip_stream);
int  rtggx_read_light_list(rtggx_context* ctx, RtggxLight* out, size_t bytes);
int  rtggx_read_light_list_rejects(rtggx_context* ctx, uint64_t* rejects, int reset);
int  rtggx_debug_visibility_drains(rtggx_context* ctx, uint32_t* drains, int reset);

/* The sun from the environment: finds the sun in the current cube, measures its direction and irradiance -- what rtggx_set_sun wants -- and,
 * where asked, takes it out of the cube, so that a probe with a sun in it does not light the scene twice (once analytically, with shadows, and
 * once more through the environment lookups, the SH irradiance and every level of the chain).  A setup call, not per frame; opt-in: a context
 * that never calls it allocates and launches exactly what it always did.  It synchronises.  S is the cube's side, level 0 the current RGBA16F
 * level 0, and everything below is double arithmetic, each operation rounded on its own (no contraction), on values that are exact in a double.
 *   Texels.  Per channel v = x > 0 ? min(x, 65504) : 0 (NaN and negatives become 0: the image loader's rule); Y(c) = (0.25 c.r + 0.5 c.g) +
 *     0.25 c.b (exact for binary16 inputs).  Texel (f, x, y) has the index i = (f S + y) S + x and the integer direction D = S cubeFaceDir(f,
 *     a / S, b / S) with a = 2 x + 1 - S, b = 2 y + 1 - S: face 0 (S, -b, -a), 1 (-S, -b, a), 2 (a, S, b), 3 (a, -S, -b), 4 (a, -b, S),
 *     5 (-a, -b, -S).  n = D . D.  Sides above 8192 are refused; up to there D, n and every dot product of two directions are exact.
 *   Peak.  The texel of greatest Y, ties to the lowest i: peak_face, peak_x, peak_y; peak_luma its Y; P its D, nP = P . P.
 *   Masks.  dot = D . P.  A texel is IN THE CONE iff dot > 0 && dot dot >= (cos2_cone n) nP, IN THE RING iff it is not in the cone and the
 *     same holds with cos2_ring.  cos2 = c c with c = cos((double)degrees (3.14159265358979323846 / 180.0)), the host's libm; both are
 *     reported, so that a restatement uses them and not a cosine of its own.
 *   Weights.  q = sqrt(n), w = (4.0 S) / (n q) (the texel's solid angle up to a constant factor), d = D / q per component.
 *   Pass B, all texels: weight_all = sum w; sum w Y; weight_ring = sum_ring w; ring_rgb[c] = sum_ring w v_c; texels_cone, texels_ring.  Then
 *     mean_luma = (sum w Y) / weight_all; background[c] = ring_rgb[c] / weight_ring, 0 with an empty ring; b16[c] = the binary16 nearest
 *     (ties to even) to (float)background[c] capped at 65504 -- background_half reports it as a float.
 *   found = 0, and nothing further is done, when peak_luma == 0 or peak_luma < min_contrast mean_luma: an overcast sky has no sun to take out.
 *   Pass C, the cone: e_c = max(v_c - b16_c, 0); weight_cone = sum w; excess[c] = sum w e_c; moment = sum (w Y(e)) d per component;
 *     texels_lit counts the texels with e > 0 in some channel.  Then, each quantity rounded to fp32 once: direction = moment / |moment|,
 *     irradiance[c] = excess[c] (4 pi / weight_all) -- the normalisation of rtggx_transform_sh.  There is no cosine factor inside the cone.
 *     |moment| zero or not finite: found = 0.  When found == 0 direction and irradiance are 0.
 *   THE ORDER OF EVERY SUM IS FIXED as in RtggxScore: the terms of ALL texels by i -- a texel outside the sum's mask adds +0.0 --, padded with
 *     +0.0 to a power of two, added pairwise, adjacent pairs first.  No atomics: the record depends on the cube and the arguments alone (a
 *     moment component that sums to zero may read +0.0 or -0.0).
 *   Removal (remove != 0 and found): a new cube beside the old one.  Level 0 is a copy in which, at the texels in the cone, each of r, g, b
 *     becomes min(v_c, b16_c) -- both are binary16 values, nothing is rounded; alpha is kept --, every other texel bit for bit; below it the
 *     full box chain of rtggx_generate_env_mips, whatever the cube held there before (a prefiltered cube is to be prefiltered again by the
 *     caller).  It replaces the context's cube as rtggx_generate_env_mips does -- the still-sky runs end, the SH coefficients are to be
 *     projected again -- and removed = 1.  original = residual + e holds exactly per texel: what irradiance reports is what left the cube.
 *   Nothing removed (remove == 0 or found == 0): the context is untouched -- environment, still-sky runs, SH state -- and nothing stays allocated.
 *   Defaults (0 selects them): cone_degrees 4, ring_degrees 3 x the cone, min_contrast 16.  They are policy defaults for the caller to
 *     override, not measured values.
 *   Refused, the context keeping everything: no environment; a null out; a cone outside (0, 45]; a ring outside (cone, 89]; a min_contrast
 *     that is negative or not finite; a side above 8192.
 * tests/sunenv_ref.py restates the record and the cube. */
typedef struct RtggxSunEstimate {          /* 224 bytes: 19 doubles, 9 floats, 9 words */
  double cos2_cone, cos2_ring;             /* what the masks used */
  double peak_luma, mean_luma;             /* Y of the peak texel; sum_all(w Y) / weight_all */
  double weight_all, weight_cone, weight_ring;
  double ring_rgb[3];                      /* sum_ring(w rgb) */
  double background[3];                    /* ring_rgb / weight_ring, or 0 where weight_ring == 0 */
  double excess[3];                        /* sum_cone(w e) */
  double moment[3];                        /* sum_cone(w Y(e) d) */
  float  background_half[3];               /* background after its one rounding to binary16, as floats: b16 */
  float  direction[3], irradiance[3];      /* what to hand to rtggx_set_sun; 0 when found == 0 */
  uint32_t found, removed;                 /* 0 / 1 */
  uint32_t peak_face, peak_x, peak_y;
  uint32_t texels_cone, texels_ring, texels_lit;   /* lit: in the cone with e > 0 in some channel */
  uint32_t pad;                            /* 0 */
} RtggxSunEstimate;
int  rtggx_sun_from_env(rtggx_context* ctx, float cone_degrees, float ring_degrees, float min_contrast, int remove, RtggxSunEstimate* out);

#ifdef __cplusplus
}
#endif
#endif /* RTGGX_H */
