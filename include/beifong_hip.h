/*
 * beifong_hip.h — flat C ABI of the MI355X radar path-tracing core
 * (libbeifong_hip.so).  This is the drop-in boundary for beifong's
 * transient-radar hot path:
 *
 *   SamplingIntegrator::render / render_sample   src/librender/integrator.cpp:58-310
 *   SamplingIntegrator::receive / receive_sample src/librender/integrator.cpp:315-768,1538-1667
 *   PathIntegrator::sample                       src/integrators/path.cpp:100-226
 *   PathLengthIntegrator / RangeIntegrator       src/integrators/pathlength.cpp:114-337, range.cpp:89-190
 *   PathTimeIntegrator / TimeIntegrator          src/integrators/pathtime.cpp:114-302, time.cpp:86-190
 *   PathTimeFrequencyIntegrator::sample          src/integrators/pathtimefrequency.cpp:103-460
 *   Scene::ray_intersect / ray_test              src/librender/scene.cpp:129-178
 *   ImageBlock::put / SignalBlock::put           src/librender/imageblock.cpp:79+, signalblock.cpp:79-172
 *
 * The reference's plugin ABI is C++ templates over enoki types and cannot be
 * bound binary-for-binary; the host layer (beifong_amd/host) keeps the
 * source-level plugin surface and flattens a loaded scene into the POD
 * description below.  Everything that crosses this boundary is plain C:
 * pointers, sizes, integer status codes.  No exceptions, no torch types.
 *
 * Ownership: the caller owns every input array for the duration of
 * bf_scene_create (they are deep-copied to the device) and owns every output
 * buffer.  A bf_scene handle runs ONE render at a time (it owns the path pool
 * the render's state lives in); concurrent renders of one scene on several
 * streams use one handle each — bf_scene_clone shares the geometry.  This is
 * enforced, not just asked for: a second HOST THREAD entering a call on a
 * handle that is inside one gets BF_ERR_INVALID, and a call whose stream
 * differs from the handle's previous call waits (on the device) for that
 * call's work, so successive renders of one handle are always ordered.
 *
 * Conventions: all arithmetic fp32, indices uint32, RNG state uint64.
 * Matrices are row-major float[16].  Spectra are a single grey lane (all
 * radar scenes use uniform spectra; see DESIGN.md "Spectrum").
 */
#ifndef BEIFONG_HIP_H
#define BEIFONG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BF_ABI_VERSION 5

typedef int bf_status;
enum {
    BF_OK = 0,
    BF_ERR_INVALID = 1,   /* bad argument / inconsistent description        */
    BF_ERR_DEVICE = 2,    /* HIP runtime failure (message in bf_last_error)  */
    BF_ERR_NOMEM = 3,
    BF_ERR_UNSUPPORTED = 4
};

/* ---------------- materials: BSDF plugins flattened ----------------------
 * diffuse.cpp:78-135, roughconductor.cpp:145-392, twosided.cpp:62-180 */
enum { BF_BSDF_DIFFUSE = 0, BF_BSDF_ROUGHCONDUCTOR = 1, BF_BSDF_NULL = 2 };
enum { BF_MF_BECKMANN = 0, BF_MF_GGX = 1 };

typedef struct bf_material {
    uint32_t type;           /* BF_BSDF_*                                    */
    uint32_t twosided;       /* 1: wrapped in <bsdf type="twosided">         */
    float reflectance;       /* diffuse: reflectance; conductor: specular_reflectance */
    float alpha_u, alpha_v;  /* roughconductor roughness                     */
    uint32_t distribution;   /* BF_MF_*                                      */
    uint32_t sample_visible; /* roughconductor sample_visible (default 1)    */
    float eta, k;            /* conductor complex IOR (defaults 0, 1)        */
    uint32_t has_specular_reflectance;
    uint32_t back_material;  /* twosided with TWO nested BSDFs (twosided.cpp:62-92: the second one shades the back side):
                                0 = the same BSDF on both sides; k + 1 = table entry k (itself twosided, back_material 0)
                                is used when the incident direction is below the surface                            */
} bf_material;

/* ---------------- shapes ------------------------------------------------- */
enum { BF_SHAPE_RECTANGLE = 0, BF_SHAPE_MESH = 1 };

typedef struct bf_shape {
    uint32_t type;           /* BF_SHAPE_*                                   */
    uint32_t material;       /* index into materials                         */
    int32_t  emitter;        /* index into emitters if an area emitter / surface
                                transmitter is attached, else -1             */
    uint32_t is_sensor;      /* shape carries the sensor / receiver          */
    /* rectangle (src/shapes/rectangle.cpp): unit square [-1,1]^2, z=0.
       The reference's Transform carries its own inverse (transform.h), so the
       host layer supplies both; the core never inverts a matrix.            */
    float to_world[16];
    float to_object[16];
    /* mesh (include/mitsuba/render/mesh.h:344-348): world-space vertices
       (to_world already applied, as obj.cpp / ply.cpp do at load time)      */
    const float *positions;  /* [3 * n_vertices]                             */
    const float *normals;    /* [3 * n_vertices] or NULL                     */
    const float *texcoords;  /* [2 * n_vertices] or NULL: with them dp_du follows the
                                UV parameterisation (mesh.cpp:493-512) instead of
                                coordinate_system(n), which turns the shading frame */
    const uint32_t *indices; /* [3 * n_faces]                                */
    uint32_t n_vertices;
    uint32_t n_faces;
    /* Shape "velocity" transform (src/librender/shape.cpp:42, default identity) read by
       Shape::doppler (shape.cpp:375-389); only used with BF_FLAG_DOPPLER.  All zeros = identity. */
    float velocity[16];
} bf_shape;

/* ---------------- emitters / transmitters -------------------------------- */
enum {
    BF_EMITTER_SPOT = 0,         /* src/emitters/spot.cpp:64-170             */
    BF_EMITTER_AREA = 1,         /* src/emitters/area.cpp:64-150             */
    BF_TRANSMITTER_AREA = 2,     /* src/transmitters/areatransmitter.cpp     */
    BF_TRANSMITTER_WIGNER = 3,   /* src/transmitters/wignertransmitter.cpp   */
    BF_TRANSMITTER_PHASED = 4,   /* src/transmitters/phasedtransmitter.cpp   */
    BF_EMITTER_POINT = 5         /* src/emitters/point.cpp:60-118: position = to_world
                                    translation, `radiance` = intensity       */
};
enum { BF_SIGNAL_CW = 0, BF_SIGNAL_PULSE = 1, BF_SIGNAL_LINFMCW = 2 };

/* Phased array (phasedtransmitter.cpp:108-165, phasedreceiver.cpp:115-172): the
 * n_elems^2 VIRTUAL elements the constructors precompute, BF_VELEM_FLOATS floats
 * each:  [0..11] m_velem_to_object (3x4 row-major),  [12..23] m_dir_to_local_velem
 * (3x4 row-major, no translation),  [24..26] m_r_dash,  [28..29] m_psi_dash (re, im),
 * the rest 0.  The host layer (plugins/phased*.cpp) and beifong_amd/scenedesc.py
 * build them. */
#define BF_VELEM_FLOATS 32
typedef struct bf_phased_array {
    const float *velems;     /* n_velems * BF_VELEM_FLOATS floats, or NULL   */
    uint32_t n_velems;       /* n_elems * n_elems                            */
    float elem_dims[3];      /* m_wid                                        */
} bf_phased_array;

typedef struct bf_emitter {
    uint32_t type;
    int32_t  shape;          /* area types: index of the carrying shape      */
    float to_world[16];      /* spot                                         */
    float to_object[16];     /* spot: trafo.inverse() (spot.cpp:153)         */
    float radiance;          /* spot: intensity; area: radiance              */
    float cutoff_angle_deg;  /* spot                                         */
    float beam_width_deg;    /* spot                                         */
    /* wigner transmitter signal model (wignertransmitter.cpp:53-146)        */
    uint32_t signal_type;
    float amplitude, freq_centre, freq_ext, pulse_len, prf, gain;
    uint32_t resample_freq;  /* m_resample_freq (:211-221, 430-441): eval / sample_direction overwrite the path's wavelength with
                                MTS_C / f * 1e9, f the signal's instantaneous frequency ("linfmcw", "cw") at the interaction's /
                                the retarded time, signal power 1; "pulse": BF_ERR_UNSUPPORTED (uninitialised in the reference) */
    bf_phased_array array;   /* BF_TRANSMITTER_PHASED                        */
} bf_emitter;

/* ---------------- sensor / receiver + film / adc ------------------------- */
enum {
    BF_SENSOR_FLUXMETER = 0,     /* src/sensors/fluxmeter.cpp:63-105         */
    BF_SENSOR_PERSPECTIVE = 1,   /* src/sensors/perspective.cpp:95-199       */
    BF_RECEIVER_OMNI = 2,        /* src/receivers/omnidirectional.cpp:51-139 */
    BF_RECEIVER_WIGNER = 3,      /* src/receivers/wignerreceiver.cpp:43-299  */
    BF_RECEIVER_PHASED = 4,      /* src/receivers/phasedreceiver.cpp         */
    BF_SENSOR_IRRADIANCEMETER = 5, /* src/sensors/irradiancemeter.cpp:63-105: the flux
                                     meter's rays, weight pi / surface_area      */
    BF_SENSOR_RADIANCEMETER = 6   /* src/sensors/radiancemeter.cpp:49-114: ONE ray from
                                    to_world * origin along to_world * +z, weight 1 */
};

/* Reconstruction filter of the film / ADC (include/mitsuba/core/rfilter.h:10,55-66, src/libcore/rfilter.cpp:9-21).  The
 * host evaluates the filter (src/rfilters/{box,tent,gaussian,mitchell,catmullrom,lanczos}.cpp) into the reference's
 * discretisation; the kernels only look the table up, exactly as ImageBlock::put / SignalBlock::put do
 * (imageblock.cpp:109-165, signalblock.cpp:111-161): eval_discretized(x) = values[min(int(|x * scale|), 31)].
 * radius <= 0.5 + RayEpsilon (e.g. the zero-initialised struct) selects put()'s box branch — one pixel, weight 1 — and
 * nothing else of the struct is read.                                                                                   */
#define BF_FILTER_RESOLUTION 31              /* MTS_FILTER_RESOLUTION */
typedef struct bf_rfilter {
    float radius;                            /* m_radius                                                  */
    float scale;                             /* m_scale_factor = MTS_FILTER_RESOLUTION / m_radius          */
    uint32_t border;                         /* m_border_size = ceil(radius - .5 - 2 RayEpsilon)           */
    uint32_t block_size;                     /* render(): edge of the image blocks a film is rendered in (integrator.cpp:
                                                101-114, MTS_BLOCK_SIZE 32); a sample's position is taken relative to ITS
                                                block's offset - border (imageblock.cpp:113), which matters to the last bit
                                                only.  0: the film / ADC is one block (receive(): integrator.cpp:624-627)  */
    float values[BF_FILTER_RESOLUTION + 1];  /* m_values; values[31] = 0                                   */
} bf_rfilter;

typedef struct bf_sensor {
    uint32_t type;
    int32_t  shape;          /* fluxmeter / receivers: carrying shape        */
    float to_world[16];      /* perspective: camera-to-world                 */
    float sample_to_camera[16]; /* perspective: m_sample_to_camera
                                   (perspective.cpp:104-109, sensor.h:196-231) */
    float fov_x_deg;         /* perspective (already resolved to the x axis) */
    float near_clip, far_clip;
    uint32_t film_width, film_height;     /* the film's CROP size (film.cpp:22-27; = its size without a crop window): what
                                             the sensor samples, the launch names and the histogram holds               */
    float shutter_open, shutter_open_time;
    /* receiver / ADC (receiver.cpp:16-62, adc.cpp:18-46)                    */
    float adc_sampling_start, adc_sampling_time;
    uint32_t t_bins, f_bins;               /* the ADC's FULL size: tf is scaled by size / bandwidth (integrator.cpp:1639)   */
    float t_bandwidth, f_bandwidth;
    float freq_centre, freq_ext, gain;     /* wigner receiver                */
    uint32_t rx_sig_is_delta;  /* wignerreceiver.cpp:258 reads an uninitialised
                                  m_sig_is_delta in raw mode; made explicit  */
    bf_phased_array array;   /* BF_RECEIVER_PHASED                           */
    bf_rfilter rfilter;      /* film->reconstruction_filter() / adc->reconstruction_filter() */
    /* ADC window (adc.cpp:26-38, set_window :80-91): receive() bins into a SignalBlock of window size at the window's offset
     * (integrator.cpp:627-628) and the ADC stores just that (hdradc.cpp:166-167): the histogram of a receive-mode launch is
     * [window_f_bins][window_t_bins][channels] and bf_launch.bins / bins_y name the WINDOW.  All four zero: the whole ADC.      */
    uint32_t window_offset_t, window_offset_f, window_t_bins, window_f_bins;
    /* Film crop window (film.cpp:17-27): the offset of the crop inside the full film.  The position sample of pixel p is
     * (p + crop_offset) + next_2d and the sensor takes (position - crop_offset) / crop_size (integrator.cpp:263,276-278); a
     * perspective camera's sample_to_camera already contains the crop (sensor.h:196-231).  Both zero without a crop window.   */
    uint32_t crop_offset_x, crop_offset_y;
    /* Wigner / phased receiver under receive_type "mix_resample" (BF_FLAG_MIX_RESAMPLE): the receiver samples its frequency from a
     * local-oscillator signal of its own (wignerreceiver.cpp:72-110, sample_frequency :172-189, sample_delta_frequency :149-166):
     * BF_SIGNAL_LINFMCW — the chirp's instantaneous frequency freq_centre + (freq_ext / rx_pulse_len) * (t - rx_pulse_len / 2),
     * t = fmodulo(time, 1 / rx_prf), freq_ext the sweep — or BF_SIGNAL_CW (freq_centre), at the sampled receive time, weight 1
     * (sig_is_delta, the plugins' default for both).  Against a resample_freq transmitter the ADC's frequency axis is then the
     * de-chirped beat.  A signal that is NO delta (rx_sig_is_delta = 0: the plugins' default for "pulse") draws the frequency
     * uniformly from [freq_centre - freq_ext / 2, freq_centre + freq_ext / 2] and weights the ray with eval_signal(time, f)
     * (:118-142: the chirp's / pulse's Wigner function with rx_amplitude, or rx_amplitude^2 for "cw").  "pulse" as a delta reads an
     * uninitialised frequency in the reference: BF_ERR_UNSUPPORTED.  Not read in the "raw" receive types; the omnidirectional
     * receiver has no signal.  */
    uint32_t rx_signal_type;
    float rx_pulse_len, rx_prf, rx_amplitude;
} bf_sensor;

/* ---------------- scene --------------------------------------------------- */
typedef struct bf_physics {
    float c;                 /* MTS_C (spectrum.h:32-35); gen-1 uses 3.0e8   */
    float lambda_min_nm;     /* MTS_WAVELENGTH_MIN (spectrum.h:15-21)        */
    float lambda_max_nm;     /* MTS_WAVELENGTH_MAX (spectrum.h:23-29)        */
} bf_physics;

typedef struct bf_scene_desc {
    const bf_shape *shapes;       uint32_t n_shapes;
    const bf_material *materials; uint32_t n_materials;
    const bf_emitter *emitters;   uint32_t n_emitters;
    bf_sensor sensor;
    bf_physics physics;
} bf_scene_desc;

typedef struct bf_scene bf_scene;   /* opaque, device resident */

/* ---------------- launch --------------------------------------------------- */
enum {
    BF_MODE_PATH = 0,         /* path.cpp; channels X,Y,Z,A,W                 */
    BF_MODE_RANGE = 1,        /* range.cpp o pathlength.cpp; +bins channels   */
    BF_MODE_TIME = 2,         /* time.cpp o pathtime.cpp; +3*bins channels    */
    BF_MODE_RECEIVE_RAW = 3,  /* receive() o pathtimefrequency.cpp; Y,A,W     */
    BF_MODE_RECEIVE_IQ = 4    /* as RECEIVE_RAW, but every contribution is a phasor
                                 c * exp(-j 2 pi L / lambda) of its own optical length L
                                 (receiver -> ... -> transmitter); ADC cells hold I, Q, W.
                                 Coherent pulse sweeps (range-Doppler); the
                                 reference has no counterpart: parity is to the oracle */
};
enum { BF_COLOR_RGB = 0, BF_COLOR_MONO = 1 };

typedef struct bf_launch {
    uint32_t mode;            /* BF_MODE_*                                    */
    uint32_t color_mode;      /* BF_COLOR_*: scalar_rgb -> XYZ via srgb_to_xyz */
    uint64_t n_paths;         /* paths rendered by THIS call                  */
    uint64_t path_offset;     /* first global path index (multi-GPU sharding) */
    uint64_t seed;            /* sampler base seed (sampler.cpp:83-96)        */
    int32_t  max_depth;       /* -1 = infinite (integrator.cpp:1713-1728)     */
    int32_t  rr_depth;        /* default 5                                    */
    uint32_t bins;            /* range/time bins; receive: ADC t_bins         */
    uint32_t bins_y;          /* receive: ADC f_bins (else ignored)           */
    float    bin_width;       /* dr [m] (range) or dt [s] (time)              */
    float    time_c;          /* gen-1 divides by (Float)3.0e8 (pathtime.cpp:140) */
    uint32_t flags;           /* BF_FLAG_*                                    */
    uint32_t phase_bins;      /* receive mode: PhaseIntegrator AOVs S{k}.Y after Y,A,W
                                 (phase.cpp:80-141); 0 = plain pathtimefrequency */
    /* Film of the render modes (integrator.cpp:58-204, Film::crop_size with crop_offset 0):
     * global path g (= path_offset + local index) samples pixel g / spp,
     * pixels in row-major order as in the reference's wavefront branch (integrator.cpp:171-187);
     * its film position is pixel + next_2d and, under the box filter, it lands in pixel ceil(pos - 1)
     * per axis (ImageBlock::put, imageblock.cpp:166-172); a wider reconstruction filter
     * (bf_sensor.rfilter) spreads it over the pixels within its radius (imageblock.cpp:115-165).
     * The histogram becomes
     * [film_height][film_width][channels].  spp == 0 (or a 0 x 0 film) means the 1 x 1 film of
     * the radar scenes: every path samples pixel 0.  path_offset + n_paths must not exceed
     * film_width * film_height * spp.  Receive modes have an ADC instead and need these 0 or 1. */
    uint32_t film_width, film_height;
    uint32_t spp;
} bf_launch;

enum {
    BF_FLAG_STATS = 1u,       /* count BVH nodes visited / triangles tested   */
    BF_FLAG_GLOBAL_ATOMICS = 2u, /* skip LDS privatisation (debug / ablation) */
    BF_FLAG_MEGAKERNEL = 4u,   /* single persistent megakernel instead of the
                                  wavefront pipeline (ablation; same results) */
    BF_FLAG_MIX_RESAMPLE = 16u, /* receive modes: receive_type "mix_resample" (integrator.cpp:1588-1603): the ADC's frequency
                                  coordinate is the BEAT frequency |c / lambda_after - c / lambda_rx| between the wavelength the
                                  path ends with and the one the receiver sampled, instead of c / lambda ("raw" / "raw_resample",
                                  :1604-1623).  The two differ by the Doppler hook (without it the beat is exactly 0 and every
                                  sample falls outside the ADC, ceil(0 - 1) = -1, as at the reference's HEAD) and by resample_freq
                                  transmitters (bf_emitter): the beat of the transmitter's instantaneous frequency with what the
                                  receiver sampled — uniformly from the band (omnidirectional) or from its own local oscillator
                                  (Wigner / phased receiver: bf_sensor.rx_signal_type ..., delta signals only).
                                  receive_type "mixer" (:1624-1634) is an empty branch there and has no counterpart here. */
    BF_FLAG_ROLLING = 32u,     /* bf_render_device only: the render joins the handle's ROLLING SEQUENCE (below, bf_scene_flush) */
    BF_FLAG_TIMING = 64u,      /* rolling sequences: HIP events around every kernel launch; bf_scene_flush's statistics carry
                                  the per-kernel sums (trace_ms / shade_ms / tail_ms).  Set it on every render of the sequence. */
    BF_FLAG_FAST = 256u,       /* opt-in fast arithmetic: the shading, tracing and tail kernels (and the one-kernel variant)
                                  come from a second compile of the same sources with approximate fp32 division and square
                                  root (v_rcp_f32 * a, v_sqrt_f32; no FMA contraction, the engine's own transcendentals;
                                  conversions between frequency and wavelength stay correctly rounded).
                                  Every other render is bit-identical per path to the oracle; a fast one is held to this
                                  TOLERANCE CONTRACT instead (tests/fast_contract.py):
                                  - a path AGREES with the oracle's when valid and n_rays are equal, |aux - aux_O| <=
                                    1e-5 |aux_O| and |L - L_O| <= 1e-4 |L_O| + 1e-7 max_p |L_O,p|; the share of paths that
                                    do not (a ray that grazes an edge, a Russian-roulette draw against a throughput one ulp
                                    away) is below 1 % in every tested scene;
                                  - the histogram is the fp32 sum of the fast render's own paths (same binning rule), so the
                                    total weight and n_paths are exact, and sum_c |h - h_O| stays within the rounding of the
                                    sums, 1e-4 of sum_c S_O, and what the diverged paths and the agreeing paths within
                                    1e-5 |aux_O| of a cell edge can move.
                                  Fast paths are bit-identical among themselves: stand-alone, batched, rolling (also across
                                  endpoint updates), sharded, lean or general kernels, one-kernel variant.  A rolling render
                                  whose BF_FLAG_FAST differs from the open sequence's fails with BF_ERR_INVALID and leaves the
                                  sequence intact.  bf_stats.kernel_variant carries BF_VARIANT_FAST.  The ray queries
                                  (bf_trace_closest / bf_trace_any / bf_ray_intersect) ignore the flag: always exact. */
    BF_FLAG_COUNT = 128u,      /* keep the ray / bounce / path counters of a render that returns no bf_stats of its own (a rolling
                                  sequence whose flush will be asked for statistics, the shards of bf_render_sharded_device).
                                  Implied by BF_FLAG_STATS and by a non-NULL stats_out; without any of them the counters stay
                                  zero — adding them up costs every shading launch ~10 same-line atomics per wave.  Set it on
                                  every render of a sequence. */
    BF_FLAG_MOMENT = 512u,     /* moment integrator (src/integrators/moment.cpp:33-53,87-91 around the launch's mode): next to
                                  every first-moment channel the histogram carries the sum of the SQUARED samples, so one
                                  render gives the variance of every bin.  Channel layout per pixel (render modes; A nested
                                  AOVs: 0 path, bins range, 3 bins time):
                                    X Y Z A W | nested AOVs | nested.X nested.Y nested.Z | m2_(nested AOVs) | m2_nested.X .Y .Z
                                  = 5 + 2 (A + 3) channels.  nested.XYZ is the XYZ of the UNWEIGHTED nested result (what the
                                  range / time AOVs see: no sensor weight); each m2_ addend is the fp32 product x * x of the
                                  value its first-moment channel received from that sample.  A sample whose square is not
                                  finite is dropped from ALL channels and counted in n_invalid (ImageBlock::put refuses a
                                  sample with any non-finite channel).  Under a reconstruction filter wider than a pixel the
                                  m2_ channels are filtered like every other channel (addend w * x * x).
                                  Receive modes have no counterpart in the reference; per ADC cell:
                                    RAW  Y A W [phase bins] m2_Y          IQ  I Q W m2_I m2_Q
                                  with the squares of the values added to Y, I and Q.
                                  Combines with batches, motion / deform batches, rolling sequences (also across endpoint
                                  updates), sharded renders and bf_allreduce_device (second moments add linearly),
                                  BF_FLAG_GLOBAL_ATOMICS, BF_FLAG_MEGAKERNEL, multi-pixel films, crop and ADC windows.  LDS
                                  privatisation is decided on the moment channel count.  Refused (BF_ERR_INVALID) together
                                  with BF_FLAG_FAST: the fast contract says nothing about squares.  A rolling render whose
                                  BF_FLAG_MOMENT differs from the open sequence's fails with BF_ERR_INVALID and leaves the
                                  sequence intact.  bf_stats.kernel_variant carries BF_VARIANT_MOMENT. */
    BF_FLAG_CLASSES = 1024u,   /* returns by target class: the render writes one histogram per class of the handle's class table
                                  (bf_scene_set_classes) instead of one.  The class of a path is shape_class[s], s the shape of
                                  its FIRST intersection (the one bf_path_record.valid reports; rectangles count: the ground, the
                                  antenna apertures), or miss_class if its first ray leaves the scene; or, with an arrival table
                                  (bf_scene_set_arrival_classes), the bin of its primary ray's direction; or, with a range-rate
                                  table (bf_scene_set_range_rate_classes), the bin of its first intersection's range rate along
                                  that ray.  Every sample the plain
                                  render adds to cell c goes, same addend and same binning rule, to cell c of its path's class
                                  block.  Layout [class][plain layout], each block exactly what bf_launch_channels describes;
                                  batches [render][class][plain layout]; bf_scene_launch_channels gives the floats per render.
                                  The per-path records are bit-equal to the plain render's, the blocks sum to the plain histogram
                                  up to fp32 summation order, and their A and W channels sum to the plain ones exactly.
                                  Honoured by bf_render / bf_render_batch / bf_render_motion_batch / bf_render_deform_batch and
                                  their _device forms, in all five modes, on 1 x 1 and W x H films, with crop and ADC windows
                                  and wide reconstruction filters, with BF_FLAG_GLOBAL_ATOMICS, BF_FLAG_MEGAKERNEL,
                                  BF_FLAG_STATS, BF_FLAG_DOPPLER and BF_FLAG_MIX_RESAMPLE.  LDS privatisation is decided on
                                  n_renders * n_classes * channels.  The class variants exist of the general kernels only:
                                  bf_stats.kernel_variant carries BF_VARIANT_CLASS and never BF_VARIANT_LEAN.
                                  Refused before anything is enqueued, an open rolling sequence staying intact: without a class
                                  table, or with BF_FLAG_FAST or BF_FLAG_MOMENT (per-class error bars are a follow-up):
                                  BF_ERR_INVALID; with BF_FLAG_ROLLING, by the sharded renders and by the converge renders:
                                  BF_ERR_UNSUPPORTED (deliberately out of scope: a rolling sequence's LDS window and base-channel
                                  table hold one block per render; shards and converge rounds are built on those and on moment
                                  renders). */
    BF_FLAG_AOV = 2048u,       /* aov integrator (src/integrators/aov.cpp:83-150,170-251 around the launch's mode, one nested
                                  integrator): every pixel also carries the arbitrary output variables of the handle's AOV table
                                  (bf_scene_set_aovs), taken from the SurfaceInteraction of the path's FIRST intersection (the one
                                  bf_path_record.valid reports and shading starts from); all of them are zero when the first ray
                                  leaves the scene (aov.cpp:167).  Per pixel, K = bf_aov_floats(table):
                                    X Y Z A W | the K AOV floats in table order | nested AOVs (0 path, bins range, 3 bins time) |
                                    nested.R nested.G nested.B nested.A
                                  X Y Z A W and the nested AOVs are the plain render's; nested.R = nested.G = nested.B is the
                                  unweighted nested result (what the range bins receive; one grey lane, replicated in both colour
                                  modes), nested.A is 1 for a valid first hit, else 0.  si.uv is prim_uv for rectangles and for
                                  meshes without texture coordinates; with them it is (uv0 * b0 + uv1 * b1) + uv2 * b2 per
                                  component, b0 = 1 - b1 - b2 (mesh.cpp:470-500), in plain fp32: three roundings of the products,
                                  two of the sums in that order, no contraction — the order si.p is interpolated in.  DUV_DX and
                                  DUV_DY are always 0 (interaction.h:635; aov.cpp never computes partials).
                                  Addends: the value itself under the box filter, the fp32 product w * x under a wider one, as
                                  for every other channel.  ImageBlock::put takes or drops a sample as a whole: a sample with ANY
                                  non-finite channel (an AOV value, or a radiance that turns non-finite bounces later) adds to no
                                  channel and counts in bf_stats.n_invalid.  Per-path records are bit-equal to the plain render's.
                                  bf_scene_launch_channels gives the floats per render; batches [render][that layout].
                                  Honoured by bf_render / bf_render_batch / bf_render_motion_batch / bf_render_deform_batch and
                                  their _device forms, in modes PATH, RANGE and TIME, on 1 x 1 and W x H films, with crop windows
                                  and wide filters, with BF_FLAG_GLOBAL_ATOMICS, BF_FLAG_MEGAKERNEL and BF_FLAG_STATS.  LDS
                                  privatisation is decided on the new channel count.  The AOV variants exist of the general
                                  kernels only: bf_stats.kernel_variant carries BF_VARIANT_AOV and never BF_VARIANT_LEAN.
                                  Refused before anything is enqueued, an open rolling sequence staying intact: without an AOV
                                  table, in a receive mode, or with BF_FLAG_FAST, BF_FLAG_MOMENT or BF_FLAG_CLASSES:
                                  BF_ERR_INVALID; with BF_FLAG_ROLLING, by the sharded renders and by the converge renders:
                                  BF_ERR_UNSUPPORTED (a rolling sequence's LDS window and base-channel table are laid out for the
                                  plain channels; shards and converge rounds are built on those and on moment renders). */
    BF_FLAG_EXACT_SUM = 4096u, /* exact-sum render: every histogram cell is fl(sum of its addends), the EXACT sum rounded once to fp32,
                                  nearest-even, instead of an fp32 sum in the order the atomics land.  The addends and the binning
                                  rule are the plain render's; the value of a cell is a pure function of the launch: the same bits
                                  on every run and on every route (tail or no tail, any pool size, BF_FLAG_MEGAKERNEL,
                                  BF_FLAG_GLOBAL_ATOMICS, LDS or global accumulation), and a batch is bit-identical to its
                                  stand-alone renders.  A cell is accumulated as a 576-bit fixed-point integer (nine 64-bit limbs,
                                  bit i weighs 2^(i - 149): every finite fp32 is an integer there) by relaxed integer atomics and
                                  rounded by a resolve kernel behind the launch's last kernel: subnormal results are kept, a
                                  magnitude at or above 2^128 - 2^103 is +-inf, an exact zero is +0.0.  hist_dev is accumulated
                                  into, as ever: a cell that received an addend comes back as fl(old + sum), one rounding; a cell
                                  without (non-zero) addends is not written.  Counting is exact too: W of a 1 x 1 film at 2^25
                                  paths is 33554432, where the fp32 sum stops at 16777216.  capi.exact_sum is the specification;
                                  bf_exact_sum / bf_exact_sum_host below run the same accumulator on caller-given addends.
                                  The limb cells (72 bytes per float of the launch's histogram) belong to the handle, grow on
                                  demand and are freed with it; the first exact-sum launch of a handle, or a larger one, allocates
                                  and is then not asynchronous and cannot be captured into a graph.  LDS privatisation is decided
                                  on n_renders * channels CELLS: 682 fit (C2's 261 do, a C4 shard's 4101 take global limbs, their
                                  five base channels a per-workgroup table).  Per-path records are unchanged.
                                  Honoured by bf_render / bf_render_batch / bf_render_motion_batch / bf_render_deform_batch /
                                  bf_render_skin_batch / bf_render_morph_batch and their _device forms, in all five modes, on
                                  1 x 1 and W x H films and on ADCs, with crop and ADC windows and wide filters, with
                                  BF_FLAG_GLOBAL_ATOMICS, BF_FLAG_MEGAKERNEL, BF_FLAG_STATS, BF_FLAG_COUNT, BF_FLAG_DOPPLER and
                                  BF_FLAG_MIX_RESAMPLE.  The exact-sum variants exist of the general kernels only:
                                  bf_stats.kernel_variant carries BF_VARIANT_EXACT_SUM and never BF_VARIANT_LEAN.
                                  Refused before anything is enqueued, an open rolling sequence staying intact: with BF_FLAG_FAST,
                                  BF_FLAG_MOMENT (the converge renders force it), BF_FLAG_CLASSES or BF_FLAG_AOV, or with
                                  n_paths >= 2^31 per render (the limbs' headroom): BF_ERR_INVALID; with BF_FLAG_ROLLING (the
                                  LDS window of a rolling sequence is laid out in floats) and by the sharded renders (an
                                  all-reduce of floats would round once per shard; reducing limbs is the follow-up):
                                  BF_ERR_UNSUPPORTED; limb cells that cannot be allocated: BF_ERR_NOMEM. */
    BF_FLAG_DOPPLER = 8u       /* receive modes: the Doppler hook the reference carries commented out
                                  ("Took doppler out to test", pathtimefrequency.cpp:124-126,141-144,180-183):
                                  the path's wavelength is shifted by Shape::doppler(si) =
                                  2 dot(si.wi, velocity * to_local(si.p)) / c * lambda (shape.cpp:388) at its first
                                  intersection and at every direct transmitter hit, and the shifted wavelength selects
                                  the ADC's frequency row.  Off by default, as at the reference's HEAD. */
};

/* per-path record for exact parity tests (optional output) */
typedef struct bf_path_record {
    float L;                  /* sensor-weighted grey radiance of the path    */
    float aux;                /* pathlength [m] / pathtime [s] / receive time */
    uint32_t valid;           /* first hit valid (alpha)                      */
    uint32_t n_rays;          /* closest + any-hit queries issued             */
} bf_path_record;

typedef struct bf_stats {
    uint64_t n_paths;
    uint64_t n_rays_closest;
    uint64_t n_rays_shadow;
    uint64_t n_nodes_visited;  /* only with BF_FLAG_STATS                     */
    uint64_t n_tris_tested;    /* only with BF_FLAG_STATS                     */
    uint64_t n_invalid;        /* samples dropped by ImageBlock::put's checks */
    uint64_t n_bounces;        /* path vertices shaded                        */
    float    kernel_ms;        /* HIP-event time of the whole render (all kernels) */
    float    trace_ms;         /* sum of the BVH traversal kernel launches (wf_trace) */
    float    shade_ms;         /* sum of the shading kernel launches (wf_shade)     */
    float    tail_ms;          /* tail kernel                                       */
    uint32_t n_launches_trace; /* wf_trace launches in this render                  */
    uint32_t n_bounce_iters;   /* wavefront iterations executed                     */
    uint64_t n_rays_tail;      /* rays traced by the tail kernel (not by wf_trace)   */
    uint64_t n_rays_traced;    /* rays that entered wf_trace (the others were resolved
                                  by wf_shade: rectangles + BVH root-box test)       */
    uint64_t n_nodes_lds;      /* of n_nodes_visited: served from wf_trace's LDS copy of
                                  the tree's top levels (only with BF_FLAG_STATS)     */
    /* per-kernel breakdown (what bench.py prices each kernel's roofline entry with) */
    uint64_t n_nodes_tail;     /* four-wide node visits of the tail kernel (BF_FLAG_STATS)   */
    uint64_t n_wnodes_tail;    /* sixteen-wide (512-byte) node visits of the tail kernel's row
                                  traversal (BF_FLAG_STATS); included in n_nodes_visited      */
    uint64_t n_tris_tail;      /* triangle tests of the tail kernel (BF_FLAG_STATS)           */
    uint64_t n_bounces_tail;   /* vertices shaded by the tail kernel                          */
    uint64_t n_shade_loads;    /* path-state rows wf_shade read                               */
    uint64_t n_shade_stores;   /* path-state rows wf_shade wrote back                         */
    uint64_t n_shade_shadow;   /* shadow requests wf_shade queued                             */
    uint64_t n_shade_rays;     /* rays generated by wf_shade (rectangle + root-box test each) */
    uint64_t n_guard;          /* rays dropped by wf_trace's iteration guard: always 0, else the
                                  render call fails with BF_ERR_DEVICE                        */
    uint32_t n_launches_tail;  /* tail kernel launches (timed renders / sequences)            */
    uint32_t n_launches_shade; /* wf_shade launches (timed renders / sequences: a rolling call has one more than
                                  bounce iterations, its wake launch)                          */
    uint32_t kernel_variant;   /* which build of the shading / tail kernels ran: BF_VARIANT_LEAN = scene and launch fit the
                                  lean profile (one area-type emitter, perspective camera or omnidirectional receiver, 1 x 1
                                  film, ...: every radar scene of the reference) and everything else is compiled out of the
                                  kernels; BF_VARIANT_WIDE = reconstruction filter wider than a pixel; 0 = general kernels.
                                  Same results either way (BF_LEAN=0 in the environment forces the general ones).  ORed with
                                  BF_VARIANT_FAST when the fast-arithmetic build ran (BF_FLAG_FAST) and with BF_VARIANT_MOMENT
                                  when the kernels' second-moment variants ran (BF_FLAG_MOMENT); BF_VARIANT_CLASS = the class
                                  variants ran (BF_FLAG_CLASSES: general kernels, so never with BF_VARIANT_LEAN); BF_VARIANT_AOV =
                                  the AOV variants ran (BF_FLAG_AOV: likewise); BF_VARIANT_EXACT_SUM = the exact-sum variants ran
                                  (BF_FLAG_EXACT_SUM: likewise)                                                                */
    uint32_t reserved_;
} bf_stats;
enum { BF_VARIANT_LEAN = 1, BF_VARIANT_WIDE = 2, BF_VARIANT_FAST = 4, BF_VARIANT_MOMENT = 8, BF_VARIANT_CLASS = 16, BF_VARIANT_AOV = 32,
       BF_VARIANT_EXACT_SUM = 64 };

typedef struct bf_scene_info {
    uint32_t n_shapes, n_rects, n_triangles, n_bvh_nodes;
    uint32_t node_bytes, tri_bytes;
    uint64_t device_bytes;
    float bbox_min[3], bbox_max[3];
    uint32_t bvh_depth;       /* levels of the four-wide tree                  */
    uint32_t bvh_stack_need;  /* worst-case traversal stack entries (<= 93)    */
    uint32_t trace_node_bytes; /* bytes per node as the throughput traversal kernel (wf_trace) reads them: node_bytes (128,
                                  fp32 child boxes) by default, 64 with the opt-in quantised nodes (BF_QUANT_BVH=1) */
    int32_t  device;          /* HIP device the scene lives on (the current device when it was created)              */
} bf_scene_info;

/* ---------------- entry points --------------------------------------------- */
/* ABI handshake.  bf_version() is BF_ABI_VERSION as the LIBRARY was compiled and bf_abi_sizeof(k) the size of struct k
 * there; a caller compares both with its own build before the first call (BF_ABI_MATCHES below; the host layer, every
 * plugin and the ctypes binding do) — a component built against an older header would otherwise have the library
 * write a larger bf_stats / read a larger bf_launch than the caller allocated. */
enum {
    BF_ABI_MATERIAL = 0, BF_ABI_SHAPE, BF_ABI_EMITTER, BF_ABI_SENSOR, BF_ABI_SCENE_DESC, BF_ABI_LAUNCH,
    BF_ABI_PATH_RECORD, BF_ABI_STATS, BF_ABI_SCENE_INFO, BF_ABI_BATCH, BF_ABI_STRUCTS
};
uint32_t bf_abi_sizeof(uint32_t which);          /* 0 for an unknown index */
/* the caller's side of the handshake: a word every component compiled against THIS header agrees on */
#define BF_ABI_FINGERPRINT                                                                                              \
    ((uint64_t) BF_ABI_VERSION << 48 ^ (uint64_t) sizeof(bf_launch) << 36 ^ (uint64_t) sizeof(bf_stats) << 24 ^        \
     (uint64_t) sizeof(bf_scene_desc) << 12 ^ (uint64_t) sizeof(bf_shape) << 6 ^ (uint64_t) sizeof(bf_emitter) ^        \
     (uint64_t) sizeof(bf_scene_info) << 18 ^ (uint64_t) sizeof(bf_batch) << 30)
uint64_t bf_abi_fingerprint(void);               /* BF_ABI_FINGERPRINT as the library was compiled */
int bf_version(void);
const char *bf_last_error(void);                 /* thread-local              */
int bf_device_count(void);
bf_status bf_set_device(int device);

bf_status bf_scene_create(const bf_scene_desc *desc, bf_scene **out);
bf_status bf_scene_destroy(bf_scene *scene);

/* Move / retune the endpoints of an existing scene WITHOUT rebuilding the BVH:
 * `desc` must describe the same layout (shape, rectangle, emitter, material
 * and triangle counts; the mesh arrays are not read) — rectangle transforms,
 * emitters / transmitters, the sensor / receiver + ADC, materials and physics
 * are replaced.  This is one frame of the reference's sweep loops, which
 * rebuild the whole scene per frame just to rotate the radar
 * (python_scripts/animated_trans_rad.py:307-373, Receive.ipynb cell 30).
 * Stream-ordered: renders enqueued on `stream` afterwards see the new
 * endpoints; renders of this scene on other streams must have completed.
 * Fails with BF_ERR_UNSUPPORTED if an endpoint moves further from the origin
 * than the bound the BVH boxes were padded for (recreate the scene then).
 * An open rolling sequence (BF_FLAG_ROLLING, below) on the same stream is NOT
 * finished first: the update joins it — the renders issued so far keep the
 * endpoints they were issued with (every path reads the tables of its own
 * render), the ones issued afterwards see the new ones — so a sweep whose
 * radar turns every frame is one sequence with one tail.  Scenes with phased
 * arrays or a reconstruction filter wider than a pixel, another stream, or
 * the 255th update of a sequence flush it instead (same results). */
bf_status bf_scene_update_endpoints(bf_scene *scene, const bf_scene_desc *desc, void *stream);

/* Rigidly translate ALL mesh triangles of the scene to `offset` (metres, relative
 * to the positions the scene was created with — absolute, so a sweep does not
 * accumulate rounding): vertices become fl(p0 + offset), the four-wide BVH is
 * re-fitted in place (boxes shifted and re-padded), rectangles and endpoints
 * stay.  A moving target between the pulses of a coherent sweep (SURVEY 8f-1;
 * the reference rebuilds the scene per frame, animated_trans_rad.py:307-373).
 * Stream-ordered like bf_scene_update_endpoints. */
bf_status bf_scene_translate_meshes(bf_scene *scene, const float offset[3], void *stream);

/* Rigidly move every mesh shape k to to_world[12*k .. 12*k+11] (3x4 row-major [R | t]), ABSOLUTE — relative to the
 * vertices the scene was created with.  Entry k of a non-mesh shape must be the identity.  Each mesh moves on its own
 * (two targets at different speeds, a turning car): the four- and sixteen-wide BVHs are re-fitted bottom-up on the
 * device (same topology, boxes recomputed from the moved triangles), no rebuild.  DESIGN.md 6d.
 *   Positions: p'.x = fl(fl(fl(fl(r00 x) + fl(r01 y)) + fl(r02 z)) + t0), the same for y and z — every product and sum
 *     rounded in fp32, no FMA (beifong_amd/motion.py: apply_rigid is the same expression in numpy).  A shape whose
 *     entry is exactly the identity keeps its vertices bit for bit.
 *   Vertex normals: n' = R n0 in the same order, without t and not renormalised.  The triangle records' prim / shape
 *     / tag words and the texture coordinates are untouched.
 *   Equivalence: every path renders bit-identically to a bf_scene_create of the same description with the moved
 *     position and normal arrays, in every mode (range, time, receive, IQ, BF_FLAG_FAST, batches, rolling sequences,
 *     shards, the one-kernel variant), and bf_ray_intersect returns the same hits.
 *   Validation: rigid only — |R^T R - I|_inf <= 1e-5 and det R > 0 — else BF_ERR_INVALID; also BF_ERR_INVALID for a
 *     non-finite entry, a non-identity entry of a non-mesh shape and n_shapes != the scene's shape count.  A
 *     non-identity entry for a mesh that carries an emitter / transmitter gives BF_ERR_UNSUPPORTED (its sampling tables
 *     were built from the triangles as created; receivers and sensors sit on rectangles).  The error text names the
 *     shape.  A call that fails leaves the scene exactly as it was.
 *   With bf_scene_translate_meshes: both calls are absolute from the geometry as created and the latest call of either
 *     kind defines the geometry (translate(o) after a transform puts every mesh at p0 + o, normals as created).
 *     Batched mesh_offsets apply on top of the current geometry: fl(p' + off).
 *   Stream-ordered like bf_scene_translate_meshes; an open rolling sequence on the handle is finished first.  A handle
 *     that shares its geometry with clones copies on write (triangles, nodes, vertex normals); a clone of a moved handle
 *     starts from the geometry that handle renders at that moment.  The first call on a handle reads the tree's
 *     topology and every mesh's box back once.  The bound on ray origins the boxes are padded for is raised to cover
 *     the moved meshes (never lowered).  bf_scene_info.bbox_* keeps reporting the box as created. */
bf_status bf_scene_transform_meshes(bf_scene *scene, uint32_t n_shapes, const float *to_world, void *stream);
/* Replace the BASE vertices of mesh shape `shape`: the positions (and vertex normals) "the scene was created with", for a
 * mesh whose vertices come out of a simulation or a skinning step each frame.  Same n_vertices, same indices: the topology
 * is fixed, so the trees are re-fitted bottom-up on the device (bf_scene_transform_meshes' level kernels), never rebuilt,
 * and the traversal stack bounds and the tail's row count stay valid; quantised nodes are re-quantised.  DESIGN.md 6d.
 *   Base replacement: the pose the handle holds (its latest bf_scene_transform_meshes / bf_scene_translate_meshes) is
 *     applied on top of the new base by the arithmetic of those calls.  No arithmetic touches the values themselves: a
 *     triangle row holds the floats given.
 *   Equivalence: after the call every path, in every mode a rigid transform supports, and every bf_ray_intersect /
 *     bf_trace_* result is bit-identical to a bf_scene_create of the same description with shape `shape` carrying
 *     `positions` (and `normals`), followed by the same transform call.
 *   Normals: NULL keeps the base normals the mesh has; non-NULL on a mesh created without normals is BF_ERR_INVALID.
 *     Normals are not recomputed unless the shape's normal mode is BF_NORMALS_RECOMPUTE (bf_scene_set_normal_mode, below): then
 *     a call with normals == NULL computes them on the device from `positions`, and the equivalence above holds with `normals`
 *     = bf_vertex_normals(positions).  Texture coordinates and the rows' prim / shape / tag words are untouched.
 *   Origin bound: the host form computes the shape's new box and raises (never lowers) the bound on ray origins the boxes
 *     are padded for.  The device form cannot see the values: the caller declares bound >= max |coordinate| of the
 *     vertices passed and [-bound, bound]^3 is taken as the shape's base box.  The gather kernel checks every corner it
 *     reads (position finite with |c| <= bound, normal finite).  A triangle with a failing corner KEEPS ITS PREVIOUS ROW
 *     and is counted; the kernel always runs to completion.  A non-zero count is reported once, as BF_ERR_DEVICE naming a
 *     shape, by bf_scene_sync or by the handle's next render (which waits for that gather's count before it enqueues
 *     anything: one event and eight bytes per device-form update); every render issued between the bad update and
 *     the report is invalid.  A deform batch reports its own violations if it is given stats_out, else the next call does.
 *   Validation, before anything is enqueued (a failed call leaves the scene as it was): BF_ERR_INVALID for a non-mesh
 *     shape, an index out of range, NULL positions, a non-finite host value, a non-positive or non-finite bound;
 *     BF_ERR_UNSUPPORTED for a mesh that carries an emitter / transmitter.  The error text names the shape.
 *   Ordering and sharing as bf_scene_transform_meshes: stream-ordered (the host arrays are free again when the call
 *     returns; device arrays must stay valid until the stream has run the call), an open rolling sequence is finished
 *     first, copy on write against clones, a clone taken afterwards starts from what the handle renders then.  The first
 *     update of a scene builds a device table of every triangle slot's three vertex indices, shared by its clones. */
bf_status bf_scene_update_vertices(bf_scene *scene, uint32_t shape, const float *positions /* host [3 * n_vertices] */,
                                   const float *normals /* host [3 * n_vertices] or NULL */, void *stream);
bf_status bf_scene_update_vertices_device(bf_scene *scene, uint32_t shape, const float *positions_dev, const float *normals_dev,
                                          float bound, void *stream);

/* Rebuild both acceleration structures ON THE DEVICE, in place, over the geometry the handle renders now (its base vertices
 * as last updated, its pose on top).  Transforms and vertex updates keep the topology the scene was created with and only
 * re-fit its boxes, so a mesh that deforms frame after frame drifts away from the tree that was built for it (slower
 * traversal, same results); this call gives the handle the tree bf_scene_create would build for the same vertices —
 * same heuristic: binned SAH, 16 bins, leaves of at most 2 triangles, the same depth bound and box padding — without a new
 * handle: pose, path pool, launch plan, endpoint tables and clones all stay.
 *   Ordering: an open rolling sequence is finished first, the call waits for the handle's last work, enqueues on `stream` and
 *     returns when the new tree is in place.  It is HOST-SYNCHRONOUS, like bf_scene_create (a few words of tree sizes are read
 *     back per level).
 *   Clones: a handle that shares geometry with clones gets its own copy (copy on write: the clones keep rendering the old
 *     arrays); a clone taken afterwards shares the rebuilt arrays as it would share a created scene's (a posed handle's clone
 *     takes its snapshot, as ever).
 *   After the call:
 *     - every path in every mode and every bf_ray_intersect / bf_trace_* result is bit-identical to what the handle produced
 *       before the call (closest hits do not depend on the accelerator), hence to bf_scene_create on the same vertices;
 *     - bf_scene_transform_meshes, bf_scene_translate_meshes, bf_scene_update_vertices(_device), motion batches and deform
 *       batches keep working: they re-fit the NEW topology;
 *     - what those calls cache lazily is invalidated or permuted with the triangle slots: the level lists are rebuilt at the
 *       next re-fit, the per-mesh boxes are kept, the vertex-index table of bf_scene_update_vertices and every per-slot row
 *       (triangles and vertex normals, posed and base, texture coordinates) move into the new leaf order, and a batch lays
 *       its geometry versions out for the new node counts;
 *     - the pose stays "absolute from the base": the next transform starts from the base vertices, not from the posed ones;
 *     - the ray-origin bound the boxes are padded for is kept, never lowered;
 *     - bf_scene_get_info reports the new n_bvh_nodes, bvh_depth and bvh_stack_need (and the current bounding box).
 *   The tree is a pure function of the triangle rows: two rebuilds of the same geometry give byte-identical arrays.
 *   A scene without mesh triangles: BF_OK, nothing happens.  scene == NULL: BF_ERR_INVALID.  If the call fails (BF_ERR_NOMEM,
 *   BF_ERR_DEVICE; BF_ERR_UNSUPPORTED if a depth or stack bound cannot be met) the scene is exactly as it was. */
bf_status bf_scene_rebuild_bvh(bf_scene *scene, void *stream);
/* Read-back of a tree for tests and tools, after the handle's last work (an open rolling sequence is finished first).
 * width 4: bf_scene_info::n_bvh_nodes nodes of 128 bytes (lo.x[4], lo.y[4], lo.z[4], hi.x[4], hi.y[4], hi.z[4], child[4], pad[4]);
 * width 16: the tail kernel's nodes of 512 bytes (16 child records of 8 words: lo.xyz, hi.xyz, reference, 0).  A child reference
 * >= 0 is a node index; < 0 is a leaf, ~ref = (first_slot << 3 | count - 1) for width 4, (first_slot << 4 | count - 1) for
 * width 16; INT32_MIN marks an unused slot.  An unused slot's box is inverted, exactly lo = +inf and hi = -inf on every axis, in the
 * tree as created and after every call that rewrites the boxes (translate, transform, vertex update, rebuild): a kernel may rely on
 * the box alone to reject it.  tri_rows_out (or NULL): the 12 floats of every triangle slot in
 * leaf order (three rows of x, y, z and a word: primitive, shape, tag).  *root_child: the root's child reference.
 * nodes_bytes too small: BF_ERR_INVALID, and bf_last_error() says "needs <n> bytes"; width 16 on a scene without the
 * sixteen-wide tree (BF_NO_WIDE_BVH, no triangles): BF_ERR_UNSUPPORTED. */
bf_status bf_scene_read_bvh(const bf_scene *scene, uint32_t width /* 4 or 16 */, void *nodes_out, uint64_t nodes_bytes,
                            float *tri_rows_out /* 12 floats per slot, or NULL */, int32_t *root_child);
bf_status bf_scene_get_info(const bf_scene *scene, bf_scene_info *info);

/* A second handle on the same scene for another stream: the big read-only arrays (BVH, triangles,
 * normals, texture coordinates) are SHARED with `scene` and freed with the last handle; the clone
 * has its own endpoint tables (rectangles, emitters / transmitters, sensor / receiver, materials —
 * bf_scene_update_endpoints on one handle does not touch the others), its own path pool and
 * counters, so renders on different handles may run concurrently on different streams.  The
 * reference shares one Scene object between its worker threads the same way
 * (src/librender/integrator.cpp:125-159: every thread renders blocks of the same scene).
 * bf_scene_translate_meshes on a handle that shares its geometry copies on write.  A clone of a
 * scene that has been translated starts from the geometry that scene renders at that moment. */
bf_status bf_scene_clone(const bf_scene *scene, bf_scene **out);

/* number of floats the given launch accumulates into: 5 (+bins | +3*bins) for
 * the 1x1 film modes, f_bins*t_bins*3 ([y=f][x=t][Y,A,W]) for receive; with
 * BF_FLAG_MOMENT the layout documented at the flag: 5 + 2 (A + 3) per pixel,
 * 4 + phase_bins (RAW) or 5 (IQ) per ADC cell */
uint32_t bf_launch_channels(const bf_launch *launch);

/* Returns by target class (BF_FLAG_CLASSES).  A scene handle carries an optional class table: n_classes, one class per shape
 * (shape_class: host array [n_shapes], shapes in the order of the scene description, rectangles included) and the class of a
 * path whose first ray leaves the scene.
 *   bf_scene_set_classes is stream-ordered like bf_scene_update_endpoints: renders enqueued afterwards on that stream see the new
 *   table; the caller's array is free on return.  It flushes an open rolling sequence.  n_classes = 0 clears the table.
 *   BF_ERR_INVALID for an entry or miss_class >= n_classes, or n_classes > BF_MAX_CLASSES.  bf_scene_clone copies the table;
 *   endpoint updates, mesh transforms, vertex updates and BVH rebuilds leave it alone.
 *   bf_scene_launch_channels returns the floats ONE render of `launch` writes on this handle: n_classes times what
 *   bf_launch_channels returns if the launch carries BF_FLAG_CLASSES and the handle a table, what bf_launch_channels returns otherwise. */
#define BF_MAX_CLASSES 256
bf_status bf_scene_set_classes(bf_scene *scene, uint32_t n_classes, const uint32_t *shape_class /* host [n_shapes] */, uint32_t miss_class,
                               void *stream);
uint32_t bf_scene_launch_channels(const bf_scene *scene, const bf_launch *launch);

/* Returns by direction of arrival: the class table's second form, the ARRIVAL TABLE.  A path starts at the receiver, so the direction d
 * of its primary ray (what the sensor or receiver hands to the path, world space) is the direction its return arrives from; the class of
 * a path is the bin of (d . axis_u, d . axis_v) in the window [u0, u1) x [v0, v1), cut into n_u x n_v bins, and n_u n_v, the LAST class,
 * for a direction outside the window: n_classes = n_u n_v + 1.  In fp32, every product and sum rounded on its own, no FMA:
 *     u  = fl(fl(fl(d.x a.x) + fl(d.y a.y)) + fl(d.z a.z))       a = axis_u; v likewise with axis_v
 *     su = fl(fl((float) n_u) / fl(u1 - u0))                      once, when the table is set; sv likewise
 *     tu = fl(fl(u - u0) * su),  tv = fl(fl(v - v0) * sv)
 *     inside = tu >= 0 && tu < (float) n_u && tv >= 0 && tv < (float) n_v          (a NaN is outside)
 *     class  = inside ? (uint32) tv * n_u + (uint32) tu : n_u * n_v
 * (csrc/bf_arrival.h is that arithmetic, capi.arrival_classes its statement in numpy.)  The axes are used as given, without
 * normalisation, and they are WORLD-SPACE: they do not follow the sensor when bf_scene_update_endpoints turns the radar; set the table
 * again for the new boresight.  The class is fixed when the path is generated: the first intersection does not change it and a path that
 * leaves the scene keeps it (there is no miss class in this form).  With the class known per path BF_FLAG_CLASSES does what it does with
 * shape classes: same layout [class][plain layout], same records, same sums, honoured and refused by the same entries with the same
 * status and message; range_doppler of block k of a sweep's cube is the range-Doppler map of angle bin k.
 *   A handle has ONE table: bf_scene_set_arrival_classes behaves as bf_scene_set_classes does (stream-ordered, the caller's struct free
 *   on return, flushes an open rolling sequence, copied by bf_scene_clone, left alone by endpoint updates, mesh transforms, vertex
 *   updates and BVH rebuilds) and each of the two calls replaces what the other installed; bf_scene_set_classes with n_classes = 0
 *   clears either.
 *   BF_ERR_INVALID for a null pointer, n_u or n_v = 0, n_u n_v + 1 > BF_MAX_CLASSES, an axis or window value that is not finite,
 *   u1 <= u0 or v1 <= v0, or a scale su / sv that is not finite. */
typedef struct bf_arrival_bins {
    float axis_u[3], axis_v[3];
    float u0, u1, v0, v1;
    uint32_t n_u, n_v;
} bf_arrival_bins;
bf_status bf_scene_set_arrival_classes(bf_scene *scene, const bf_arrival_bins *bins, void *stream);

/* Returns by range rate: the class table's third form, the RANGE-RATE TABLE.  One render then gives a range-Doppler map: block k of the
 * histogram holds the returns whose first scatterer opens its range to the radar at a rate inside bin k.
 *   Motion model: every shape, rectangles included, moves rigidly; a point p of shape k has velocity lin_k + ang_k x (p - pivot_k)
 *   (bf_twist, world space: m/s, rad/s, m), and the radar moves with sensor_lin.
 *   Inputs: p, the world-space position of the path's FIRST intersection (what bf_ray_intersect returns for the primary ray; in a batch
 *   with per-render geometry or mesh offsets, that render's geometry), and d, the direction of the primary ray, used as given.
 *   Rule, in fp32, every product, sum and difference rounded on its own, no FMA:
 *     q    = fl(p - pivot)                                          per component
 *     c.x  = fl(fl(ang.y q.z) - fl(ang.z q.y))                      c.y, c.z cyclically
 *     w    = fl(fl(lin + c) - sensor_lin)                           per component
 *     rr   = fl(fl(fl(d.x w.x) + fl(d.y w.y)) + fl(d.z w.z))
 *     sr   = fl(fl((float) n_bins) / fl(r1 - r0))                   once, when the table is set
 *     t    = fl(fl(rr - r0) * sr)
 *     class = (t >= 0 && t < (float) n_bins) ? (uint32) t : n_bins          (a NaN is outside; -0 >= 0 is inside)
 *   and a path whose first ray leaves the scene has class n_bins + 1: n_classes = n_bins + 2, [bins..., outside, miss].
 *   (csrc/bf_range_rate.h is that arithmetic, capi.range_rate_classes its statement in numpy.)  A positive rr is an OPENING range; the
 *   monostatic Doppler shift of bin centre rr is -2 rr / lambda.  The rate is taken along the RECEIVE ray only: the leg from a bistatic
 *   transmitter and every later bounce of the path do not enter; the class is fixed at the first intersection.
 *   Not bf_shape.velocity: that field is the reference's Shape "velocity" transform, applied to a point in the local frame, and belongs
 *   to BF_FLAG_DOPPLER alone; this table neither reads nor changes it.
 *   Twists and pivots are WORLD-SPACE values at the time of the render: they do not follow bf_scene_transform_meshes or the transforms
 *   of a motion batch (the point p does).
 *   A handle has ONE table: this call behaves as the other two do (stream-ordered, the caller's memory free on return, flushes an open
 *   rolling sequence, copied by bf_scene_clone, left alone by endpoint updates, mesh transforms, vertex updates and BVH rebuilds), each
 *   of the three calls replaces what another installed, and bf_scene_set_classes with n_classes = 0 clears any form.  With the class
 *   known per path BF_FLAG_CLASSES does what it does with shape classes, honoured and refused by the same entries with the same status
 *   and message.
 *   BF_ERR_INVALID for a null pointer (twists may be null only for a scene without shapes), n_bins = 0, n_bins + 2 > BF_MAX_CLASSES, a
 *   table value that is not finite, r1 <= r0, or a scale sr that is not finite. */
typedef struct bf_twist {
    float lin[3], ang[3], pivot[3];
} bf_twist;
typedef struct bf_range_rate_bins {
    float sensor_lin[3];
    float r0, r1;
    uint32_t n_bins;
} bf_range_rate_bins;
bf_status bf_scene_set_range_rate_classes(bf_scene *scene, const bf_range_rate_bins *bins,
                                          const bf_twist *twists /* host [n_shapes], scene-description order */, void *stream);

/* Range rate from per-vertex velocities: micro-Doppler under the range-rate table.  A mesh that does not move rigidly (a skinned
 * figure, a spinning wheel, a vibrating panel) carries a velocity per vertex on top of its shape's twist.
 *   bf_scene_set_velocity_mode: per handle and mesh shape.
 *     BF_VELOCITY_TWIST (the default): the rule above, bit for bit.  Rectangles are always in this mode.
 *     BF_VELOCITY_VERTEX: an explicit per-vertex field, zero until bf_scene_set_vertex_velocities gives one; every render of a batch
 *       sees the same field.
 *     BF_VELOCITY_DIFFERENCE: the corner velocities are differences of the rendered positions over the time step dt (seconds, finite
 *       and positive; ignored by the other two modes): fl(fl(P_next - P_prev) / dt) per component, IEEE fp32 division, P the
 *       world-space corner exactly as the rendered triangle holds it (after the vertex update or pose, and after the handle's rigid
 *       pose or a batch's per-render transform).
 *       On a handle every call that rewrites the shape's rendered triangles (bf_scene_update_vertices*, bf_scene_pose_skin,
 *       bf_scene_pose_morph, bf_scene_transform_meshes, bf_scene_translate_meshes) sets the field from the triangles before and after
 *       the call: a frame-by-frame sweep carries backward differences, and before the first such call the field is zero.  A vertex
 *       update or a pose moves one shape and sets that shape's field alone; a transform or a translation sets every shape's.
 *       In a motion, deform, skin or morph batch render k < n_renders - 1 takes P_prev from version k and P_next from version k + 1,
 *       and the last render takes the field of render n_renders - 2; such a batch needs n_renders >= 2 while any shape of the handle
 *       is in this mode and the launch reads velocities (BF_FLAG_CLASSES under a range-rate table; BF_ERR_INVALID otherwise), gives
 *       the same fields however BF_MOTION_BATCH_MB cuts it, and leaves the handle's own field alone, as it leaves its pose.
 *     Setting a mode other than BF_VELOCITY_TWIST zeroes the shape's field.  The call waits for the handle's work in flight.
 *   Rule: under a range-rate table, a path whose first intersection lies on a triangle of a shape in mode VERTEX or DIFFERENCE, at
 *   barycentrics (u, v) (bf_ray_intersect's prim_uv) of a triangle with corner velocities V0, V1, V2 in face order, replaces w by
 *     b0   = fl(fl(1 - u) - v)
 *     U    = fl(fl(fl(b0 V0) + fl(u V1)) + fl(v V2))                per component
 *     w    = fl(fl(fl(lin + c) + U) - sensor_lin)                   per component; lin, c: the shape's twist, as above
 *   and goes on with rr, t and the class as above: the twist still applies underneath (a walking figure is a translating twist plus
 *   a vertex field).  A field value that is not finite gives an rr that is not finite: the class outside the window.  Corner
 *   velocities are WORLD-SPACE values used as given; like twists they are not rotated by anything.  (csrc/bf_velocity.h is that
 *   arithmetic; capi.interpolate_velocity, capi.corner_velocities and capi.range_rate_classes state it in numpy.)
 *   bf_scene_set_vertex_velocities (and its _device form, which reads a device array valid until `stream` has run the call) gathers
 *   the field of a shape in BF_VELOCITY_VERTEX to its triangles: stream-ordered, the caller's memory free on return.
 *   bf_scene_rebuild_bvh carries the field along; bf_scene_clone copies modes, time steps and field.
 *   BF_ERR_INVALID for a null scene (or a null mode_out and dt_out), a shape that is not a mesh, an unknown mode, a dt that is not
 *   finite and positive in BF_VELOCITY_DIFFERENCE, a field given to a shape that is not in BF_VELOCITY_VERTEX, and a value of the
 *   host form that is not finite. */
enum { BF_VELOCITY_TWIST = 0, BF_VELOCITY_VERTEX = 1, BF_VELOCITY_DIFFERENCE = 2 };
bf_status bf_scene_set_velocity_mode(bf_scene *scene, uint32_t shape, uint32_t mode, float dt);
bf_status bf_scene_get_velocity_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out, float *dt_out /* either may be NULL */);
bf_status bf_scene_set_vertex_velocities(bf_scene *scene, uint32_t shape, const float *vel /* host [n_vertices][3], NULL: zeros */, void *stream);
bf_status bf_scene_set_vertex_velocities_device(bf_scene *scene, uint32_t shape, const float *vel_dev /* device [n_vertices][3], NULL: zeros */,
                                                void *stream);

/* Arbitrary output variables (BF_FLAG_AOV).  A scene handle carries an optional AOV table: a list of BF_AOV_* types, in the order
 * their channels follow X Y Z A W in every pixel; a type may appear more than once.
 *   bf_aov_floats returns K, the floats the list occupies per pixel (0 for an invalid list: no entry, more than BF_MAX_AOVS, an
 *   unknown type, or a null pointer); it needs no device.
 *   bf_scene_set_aovs is stream-ordered like bf_scene_set_classes: renders enqueued afterwards see the new table; the caller's
 *   array is free on return.  It flushes an open rolling sequence.  n_aovs = 0 clears the table.  BF_ERR_INVALID for an unknown
 *   type or n_aovs > BF_MAX_AOVS.  bf_scene_clone copies the table; endpoint updates, mesh transforms, vertex updates and BVH
 *   rebuilds leave it alone.
 *   bf_scene_launch_channels returns film_w * film_h * (5 + K + nested AOVs + 4) for a launch that carries BF_FLAG_AOV in a render
 *   mode on a handle with a table (the layout at the flag).
 *   An AOV launch carries its values from each path's first vertex to its end in device rows of the handle's own: the first AOV
 *   launch of a handle, and any later one that needs more of them (more path slots, a table with more components), allocates —
 *   and, growing, frees, which waits for the device — exactly as a render that grows the handle's path pool does.  Such a call
 *   is not asynchronous and cannot be captured into a graph; repeated launches of one shape are. */
enum { BF_AOV_DEPTH = 0,   /* 1 float : si.t                    */
       BF_AOV_POSITION,    /* 3       : si.p                    */
       BF_AOV_UV,          /* 2       : si.uv                   */
       BF_AOV_GEO_NORMAL,  /* 3       : si.n                    */
       BF_AOV_SH_NORMAL,   /* 3       : si.sh_frame.n           */
       BF_AOV_DP_DU, BF_AOV_DP_DV,   /* 3 each                  */
       BF_AOV_DUV_DX, BF_AOV_DUV_DY, /* 2 each: always 0 (interaction.h:635; aov.cpp never computes partials) */
       BF_AOV_TYPES };
#define BF_MAX_AOVS 16
uint32_t bf_aov_floats(uint32_t n_aovs, const uint32_t *types);
bf_status bf_scene_set_aovs(bf_scene *scene, uint32_t n_aovs, const uint32_t *types /* host [n_aovs] */, void *stream);

/* Render into a DEVICE buffer hist_dev[film_h*film_w*channels] (accumulates;
 * caller zeroes).  stream is a hipStream_t (NULL = default stream).  The call
 * is asynchronous with respect to the host unless stats_out/records are
 * requested.  This is the entry the multi-GPU driver uses: the histogram stays
 * in HBM for the RCCL reduce. */
bf_status bf_render_device(const bf_scene *scene, const bf_launch *launch,
                           float *hist_dev, bf_path_record *records_dev,
                           void *stream, bf_stats *stats_out);

/* ROLLING SEQUENCES.  Every render ends in a latency-bound tail: a few Russian-roulette survivors of 100+ bounces
 * that a nearly empty GPU finishes one dependent bounce after the other (a quarter of a 2^24-path render's time, three
 * quarters of a 2^20-path one).  Loops that render the SAME scene again and again — the accumulation passes of a long
 * Monte-Carlo render, the pulses of a coherent interval (python_scripts/animated_trans_rad.py:307-384, Receive.ipynb
 * cell 30; the reference's own sample loop is src/librender/integrator.cpp:659-663) — need not pay it per render:
 * with BF_FLAG_ROLLING, bf_render_device enqueues only the throughput part of the render and LEAVES ITS LONG PATHS ALIVE
 * in the handle's pool, where the launches of the handle's next rolling renders carry them along (a path is the same
 * path whichever launch advances it: its own PCG32 stream, sampler.cpp:83-96).  One tail runs per sequence:
 *
 *   bf_scene_flush(scene, stream, stats)   finishes every path still alive (stream-ordered; asynchronous unless
 *                                          `stats` is given).  After it — and a stream synchronisation — every
 *                                          histogram of the sequence is complete.
 *
 * Rules: the renders of a sequence share mode, n_paths (at most the handle's pool, 2^24), bins, depth limits and flags;
 * they may differ in seed, path_offset, hist_dev and records_dev (one histogram / record array PER RENDER, all of which
 * must stay valid until the flush has completed).  stats_out must be NULL.  A render that does not fit the open sequence
 * (or the 256th of a sequence), a plain or batched render, bf_scene_translate_meshes and bf_scene_clone flush the
 * sequence first (bf_scene_update_endpoints joins it where it can: see there), so no path ever sees another scene than
 * the one its render was issued for;
 * bf_scene_destroy abandons it.  Renders without the flag behave exactly as before. */
bf_status bf_scene_flush(bf_scene *scene, void *stream, bf_stats *stats_out);

/* Flush, wait for everything enqueued on the handle and report a device-side failure of ANY render since the last check:
 * a planned render (the second and later ones of a launch shape run without a host round trip) returns BF_OK before its
 * kernels have run, so wf_trace's iteration guard — dropped rays, i.e. a wrong histogram: never expected — can only be
 * reported afterwards: here (BF_ERR_DEVICE; the error refers to an EARLIER render of the handle), by the handle's next
 * render, or by a render with stats_out.  Call it at the end of a sweep. */
bf_status bf_scene_sync(bf_scene *scene);

/* ONE PROCESS, SEVERAL GPUs (SURVEY 8b "device_mask", 8e).  The reference has no multi-device path (TBB over image
 * blocks of one host, src/librender/integrator.cpp:125-159); paths are i.i.d., so GPU g of G renders the global path
 * indices bf_shard_range(launch->n_paths, g, G) of ONE render through bf_launch.path_offset — the union is the sample
 * set of a one-GPU render — and the per-GPU histograms are summed by one ncclAllReduce(float, sum) over xGMI.
 *
 *   scenes[g]   a handle of the scene created on GPU g (bf_set_device(g); bf_scene_create(...)): every entry point of
 *               this header runs on its handle's device, whatever the caller's current device is
 *   hist_dev[g] float[bf_launch_channels(launch)] on that GPU, zeroed by the caller; on completion of streams[g] it
 *               holds the histogram of the WHOLE render (all-reduced), on every GPU
 *   streams[g]  a hipStream_t of that GPU (the array, or an entry, may be NULL: default stream)
 *
 * All GPUs' launches are enqueued by the calling thread before anything is waited for.  launch->n_paths is the TOTAL.
 * With BF_FLAG_ROLLING the shards join their handles' rolling sequences and NO all-reduce is issued: flush every handle,
 * then call bf_allreduce_device on the histograms.  RCCL (librccl.so) is loaded on first use; without it the calls that
 * need a collective fail with BF_ERR_UNSUPPORTED (one GPU needs none).  bf_render_sharded is the host-buffer form
 * (histogram zeroed by the callee; statistics summed over the GPUs, times = the slowest GPU's). */
void bf_shard_range(uint64_t n_paths, uint32_t shard, uint32_t n_shards, uint64_t *offset, uint64_t *count);
bf_status bf_render_sharded_device(bf_scene *const *scenes, uint32_t n_devices, const bf_launch *launch,
                                   float *const *hist_dev, void *const *streams, bf_stats *stats_out);
bf_status bf_render_sharded(bf_scene *const *scenes, uint32_t n_devices, const bf_launch *launch,
                            float *hist_out, bf_stats *stats_out);
/* in-place sum of count floats over the GPUs `devices` (bufs[g] on devices[g]), stream-ordered on streams[g] */
bf_status bf_allreduce_device(const int *devices, uint32_t n_devices, float *const *bufs, uint64_t count,
                              void *const *streams);

/* Convenience: render into a HOST buffer (zeroed by the callee). */
bf_status bf_render(const bf_scene *scene, const bf_launch *launch,
                    float *hist_out, bf_path_record *records_out,
                    bf_stats *stats_out);

/* MANY renders of one scene in ONE launch sequence: the frames of a sweep, the pulses of a
 * coherent processing interval, the shards of a sharded render.  The reference runs such loops
 * one render() / receive() call per frame and rebuilds the scene in between
 * (python_scripts/animated_trans_rad.py:307-384, Receive.ipynb cell 30; the sample loop itself
 * is src/librender/integrator.cpp:659-663); on the GPU every render ends in a latency-bound tail
 * of a few long paths, so K renders issued one by one pay K tails.  Here render k of
 * batch->n_renders is an ordinary render of `launch` (same n_paths, path_offset, mode, bins)
 *   - with sampler seed batch->seeds[k]          (NULL: launch->seed for every render — common
 *                                                 random numbers, what a coherent sweep wants),
 *   - with all meshes at batch->mesh_offsets[3k..] (NULL: as built) — the vertices
 *     bf_scene_translate_meshes(offset) would store, added on the fly while the BVH stays put,
 *   - accumulating into hist + k * bf_launch_channels(launch),
 * and every path of every render is bit-identical to that stand-alone render.  Path records
 * (optional) are [n_renders][n_paths].  Multi-pixel films are not batched.  The arrays of
 * `batch` are host memory and are free again when the call returns. */
typedef struct bf_batch {
    uint32_t n_renders;
    const uint64_t *seeds;        /* [n_renders] or NULL                         */
    const float *mesh_offsets;    /* [n_renders][3] metres, or NULL              */
} bf_batch;
bf_status bf_render_batch_device(const bf_scene *scene, const bf_launch *launch,
                                 const bf_batch *batch, float *hist_dev,
                                 bf_path_record *records_dev, void *stream,
                                 bf_stats *stats_out);
bf_status bf_render_batch(const bf_scene *scene, const bf_launch *launch,
                          const bf_batch *batch, float *hist_out,
                          bf_path_record *records_out, bf_stats *stats_out);

/* RENDER UNTIL A RELATIVE STANDARD ERROR IS REACHED.  Every product of the engine is a Monte-Carlo histogram;
 * BF_FLAG_MOMENT gives every bin its error bar, and these entries close the loop on the device: rounds of moment renders are
 * accumulated into hist_dev until the worst significant bin is known to `target`.
 *
 *   The statistic of a BF_FLAG_MOMENT histogram (the launch's layout, flag forced on), fp64 on the device from the fp32 cells:
 *     watched pairs (m1, m2)   range / time: the A nested-AOV channels and their m2_; path: nested.Y; receive RAW: Y of every
 *                              ADC cell; receive IQ: I and Q of every cell
 *     per pair                 n = the pixel's or cell's W (a 1 x 1 film: the paths accumulated so far), mean = m1 / n,
 *                              var_of_mean = max(m2 / n - mean^2, 0) / (n - 1), rel = sqrt(var_of_mean) / |mean|
 *     significant              |m1| >= floor * max |m1| (the maximum over all watched pairs of the histogram; floor in [0, 1])
 *     stat                     max rel over the significant pairs; +inf, never NaN, when no pair is significant (max |m1| == 0),
 *                              when a significant pair has n < 2 or mean 0, or when any cell of the histogram is not finite
 *                              (n_significant is then 0)
 *   capi.converge_statistic (Python) is the same definition in float64 numpy and the specification the kernels are held to.
 *
 *   Rounds: round r (from 0) is round_renders (= R) ordinary renders of `launch` with BF_FLAG_MOMENT forced on, render j with seed
 *     launch->seed + (r R + j) * launch->n_paths (mod 2^64): ONE bf_render_batch_device call into a zeroed scratch [R][channels]
 *     of the handle for a 1 x 1 film or a receive mode (one launch sequence and one tail per round), one plain render for a
 *     multi-pixel film (R must be 1).  The seeds are n_paths apart, NOT consecutive: path p of a render draws from the stream
 *     seed + path_offset + p, so renders of seeds s and s + 1 share all but one of their paths, and an error bar over them would
 *     shrink without a new sample behind it.  n_paths apart, the renders of a call are disjoint: together they draw from the streams
 *     of paths path_offset .. path_offset + rounds R n_paths of seed launch->seed, and n, m1 and m2 of the accumulator are sums over
 *     independent samples, which is what var_of_mean assumes.  (Two calls are disjoint when their seeds are at least
 *     rounds R n_paths apart.)  The
 *     scratch blocks are then added to hist_dev in block order, one thread per cell, so the accumulator is a deterministic
 *     function of the renders, and the statistic of the accumulator after round r is written to a pinned host ring.  hist_dev
 *     [bf_launch_channels(launch | BF_FLAG_MOMENT)] is zeroed by the callee.
 *   Stop rule: the host always has one round in flight ahead of the statistic it waits for (round r + 1 is issued before stat_r
 *     is read, so the GPU never idles on the decision).  With k* the first r >= min_rounds - 1 whose stat_r <= target, the call
 *     performs exactly min(k* + 2, max_rounds) rounds (max_rounds if there is no k*), whatever the timing.  *rounds_out is that
 *     number, stat_history_out[r] (optional, [max_rounds]) the statistic after every round performed; the last entry and
 *     *n_significant_out belong to the returned histogram, which is the sum of ALL rounds performed, the look-ahead round included.
 *   The call returns when the last round's statistic has been read: it waits on that round's event (never on the device), like
 *     bf_scene_rebuild_bvh.  stats_out (optional) adds up the rounds; each round then waits for its own statistics, as a render
 *     with stats_out does.
 *   BF_ERR_INVALID before anything is enqueued (a failed call leaves the scene as it was): BF_FLAG_FAST (refused together with
 *     moments), BF_FLAG_ROLLING, target negative or NaN (+inf: stop as early as the rule permits), floor outside [0, 1],
 *     round_renders == 0, max_rounds == 0, min_rounds > max_rounds, a multi-pixel film with round_renders > 1, n_paths == 0.
 *     Launch checks are bf_render_batch_device's.  An open rolling sequence on the handle is finished first.
 *   bf_render_converge is the host-buffer form.  bf_converge_statistic_device is the statistic alone, of any moment histogram
 *     on the current device: it enqueues the kernels on `stream` and waits for their result. */
bf_status bf_render_converge_device(bf_scene *scene, const bf_launch *launch, float target, float floor, uint32_t round_renders,
                                    uint32_t min_rounds, uint32_t max_rounds, float *hist_dev, void *stream, uint32_t *rounds_out,
                                    double *stat_history_out /* [max_rounds] or NULL */, uint64_t *n_significant_out,
                                    bf_stats *stats_out);
bf_status bf_render_converge(bf_scene *scene, const bf_launch *launch, float target, float floor, uint32_t round_renders,
                             uint32_t min_rounds, uint32_t max_rounds, float *hist_out, uint32_t *rounds_out,
                             double *stat_history_out /* [max_rounds] or NULL */, uint64_t *n_significant_out, bf_stats *stats_out);
bf_status bf_converge_statistic_device(const bf_launch *launch, const float *hist_dev, float floor, double *stat_out,
                                       uint64_t *n_significant_out, void *stream);

/* A batch whose renders each move the meshes by their OWN rigid transforms: render k of n_renders renders the scene with
 * every mesh shape s at to_world[k][s] (3x4 row-major [R | t], bf_scene_transform_meshes' convention), seed seeds[k]
 * (NULL: launch->seed for every render) into hist_dev + k * bf_launch_channels(launch) and, if records_dev is not NULL,
 * records_dev + k * launch->n_paths.  One launch sequence for the whole batch, so the renders share one tail (the
 * many-target case of sweep.render_motion_sweep).  DESIGN.md 6d.
 *   Equivalence: render k is bit-identical, path for path (L, aux, valid, n_rays), to bf_scene_transform_meshes(to_world[k])
 *     followed by a stand-alone render with seed seeds[k] on a handle of the same scene, in every mode (BF_FLAG_FAST, the
 *     one-kernel variant BF_FLAG_MEGAKERNEL, BF_NO_WIDE_BVH, BF_QUANT_BVH included); histograms are the fp32 sums of those
 *     paths.  Transforms are ABSOLUTE from the geometry as created, not from the pose the handle holds now.
 *   How: one geometry version per render (moved triangles and vertex normals, re-fitted four- and sixteen-wide nodes,
 *     quantised nodes for BF_QUANT_BVH scenes), built by bf_scene_transform_meshes' kernels with a version dimension, all
 *     versions of a chunk padded for one origin bound that covers every moved mesh of the batch.  The versions live in an
 *     arena of the handle's own (never shared with clones, grown on demand, freed with the handle), capped by the
 *     environment variable BF_MOTION_BATCH_MB read at call time (default 2048 MiB); a batch that does not fit renders in
 *     consecutive chunks of renders, each its own launch sequence, with the same per-path results (at least one render
 *     per chunk, whatever the cap).
 *   The handle does not change: its own pose (transform_meshes / translate_meshes), its clones and the bound on ray
 *     origins its boxes are padded for stay as they were.
 *   Validation, before anything is enqueued (a failed call leaves the scene as it was); the error text names the render
 *     and the shape:
 *     BF_ERR_INVALID      a non-rigid, non-finite, or non-identity entry for a non-mesh shape (bf_scene_transform_meshes'
 *                         checks); n_shapes != the scene's shape count; n_renders == 0; a multi-pixel film;
 *                         BF_FLAG_ROLLING
 *     BF_ERR_UNSUPPORTED  a non-identity entry for a mesh that carries an emitter
 *   Launch checks are bf_render_batch_device's.  An open rolling sequence on the handle is finished first.
 *   Stream-ordered like bf_render_batch_device; stats_out (optional) adds up the chunks (n_paths = n_renders * n_paths). */
bf_status bf_render_motion_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders,
                                        const uint64_t *seeds, uint32_t n_shapes, const float *to_world,
                                        float *hist_dev, bf_path_record *records_dev, void *stream,
                                        bf_stats *stats_out);
/* The same with host buffers: hist_out [n_renders][channels], records_out [n_renders][n_paths] or NULL. */
bf_status bf_render_motion_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders,
                                 const uint64_t *seeds, uint32_t n_shapes, const float *to_world,
                                 float *hist_out, bf_path_record *records_out, bf_stats *stats_out);

/* The motion batch for deforming meshes: render k of n_renders sees deforming shape shapes[j] at the vertices
 * positions[j] + k * 3 * n_vertices(shapes[j]) (normals likewise, where given), every other mesh at the handle's base
 * vertices, and then every mesh at to_world[k] (NULL: no transform; else [n_renders][n_shapes][12], absolute, checked
 * as in a motion batch).  One geometry version per render in the motion batch's arena (BF_MOTION_BATCH_MB, chunking
 * unchanged), gathered, transformed and re-fitted for all renders of a chunk at once.  The handle's own base, pose and
 * clones do not change.  DESIGN.md 6d.
 *   Equivalence: render k is bit-identical, path for path, to bf_scene_update_vertices(slice k) +
 *     bf_scene_transform_meshes(to_world[k]) + a stand-alone render with seeds[k] on a second handle.
 *   bound: as bf_scene_update_vertices_device, for all arrays of the call (the host form computes it); a violation is
 *     counted and reported the same way, the triangle keeping the handle's base row in that version.
 *   Normals: a listed shape whose normals entry is NULL keeps the handle's base normals, or, under BF_NORMALS_RECOMPUTE
 *     (bf_scene_set_normal_mode), gets those of each version's untransformed positions, which to_world[k] then turns.
 *   BF_ERR_INVALID before anything is enqueued: what bf_scene_update_vertices refuses, a shape listed twice,
 *     n_renders == 0, a multi-pixel film, BF_FLAG_ROLLING, and what a motion batch refuses of to_world.  The error text
 *     names render and shape. */
bf_status bf_render_deform_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds,
                                        uint32_t n_deform, const uint32_t *shapes,
                                        const float *const *positions_dev /* [n_deform] device pointers */,
                                        const float *const *normals_dev /* NULL, or [n_deform] (entries may be NULL) */, float bound,
                                        uint32_t n_shapes, const float *to_world, float *hist_dev, bf_path_record *records_dev,
                                        void *stream, bf_stats *stats_out);
bf_status bf_render_deform_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds,
                                 uint32_t n_deform, const uint32_t *shapes, const float *const *positions /* [n_deform] host pointers */,
                                 const float *const *normals, uint32_t n_shapes, const float *to_world, float *hist_out,
                                 bf_path_record *records_out, bf_stats *stats_out);

/* Skinned meshes: linear-blend skinning on the device, the layer between rigid transforms and vertex updates.  A skin is
 * attached to a mesh shape once (rest pose, four bone indices and weights per vertex); after that a pose is n_bones 3x4
 * matrices ([R | t] row-major, any finite affine map) and the device computes the vertices.  DESIGN.md 6d.
 *   Arithmetic, fp32, every product and sum rounded (no FMA).  For a vertex with rest position x, bones i0..i3, weights w0..w3:
 *       q_k = B[i_k] x                 as bf_scene_transform_meshes evaluates a 3x4 on a point (with the translation)
 *       p'  = fl(fl(fl(fl(w0 q_0) + fl(w1 q_1)) + fl(w2 q_2)) + fl(w3 q_3))                      per coordinate
 *       n'  = the same without the translations, on the rest normal, not renormalised
 *     All four terms are always evaluated: a zero-weight slot's index must still name a bone, and there is no shortcut for
 *     an identity bone.  beifong_amd.motion.apply_skin is the numpy statement of it.
 *   bf_scene_set_skin: host arrays, deep-copied to the device.  One skin per shape; a second call replaces it, n_bones == 0
 *     removes it (the arrays are then not read).  rest_normals: given exactly if the mesh was created with vertex normals.
 *     Clones taken afterwards share the skin; a later call on either handle changes that handle alone.  The mesh itself does
 *     not move.  bf_scene_rebuild_bvh keeps skins valid (they are per vertex).
 *   bf_scene_pose_skin: the mesh's BASE becomes the skinned vertices (computed from the skin's rest arrays, whatever the base
 *     held before); the handle's pose goes on top.  Semantics, ordering, copy on write and "an open rolling sequence is
 *     finished first" are bf_scene_update_vertices': after the call every path is bit-identical to a bf_scene_create of the
 *     description with the shape carrying apply_skin's arrays, followed by the same transform call.  `bones` is a host array,
 *     free again when the call returns.  Under BF_NORMALS_RECOMPUTE (bf_scene_set_normal_mode) the blended normals n' are not
 *     computed: the shape carries bf_vertex_normals of apply_skin's positions instead, in a pose and in every version of a batch.
 *   bf_render_skin_batch(_device): bf_render_deform_batch with bones[j] = host [n_renders][n_bones(shapes[j])][12] in place
 *     of the vertex arrays.  Render k is bit-identical to bf_scene_pose_skin(slice k) + bf_scene_transform_meshes(to_world[k])
 *     + a stand-alone render with seeds[k] on a second handle.  Arena, chunking (BF_MOTION_BATCH_MB) and launch flags
 *     (BF_FLAG_CLASSES, BF_FLAG_AOV, BF_FLAG_MOMENT, BF_FLAG_FAST) as a deform batch; the handle's base, pose and clones do
 *     not change.
 *   Scratch: the posed vertices of a pose or of a batch chunk are written to a buffer of the handle's own before they are
 *     gathered into triangle rows: 12 bytes per vertex and version, 24 for a mesh with vertex normals, over the skinned
 *     shapes of the call and the renders of the largest chunk.  It grows only, is freed with the handle, and lies OUTSIDE
 *     the BF_MOTION_BATCH_MB budget.
 *   Bound: the library derives bound >= max |posed coordinate| on the host, from the rest pose's extent, the bone tables and
 *     the weight sums, and uses it where the device forms of vertex updates take the caller's; the gather checks it as a
 *     safety net (bf_scene_sync reports a violation).  Bones so large that the bound is not finite are refused.
 *   Validation, before anything is enqueued (a failed call leaves the scene as it was; the text names shape, vertex or bone):
 *     BF_ERR_INVALID      a shape index out of range or not a mesh; NULL arrays; n_bones > 256; a non-finite rest, weight or
 *                         bone value; a bone index >= n_bones; a negative weight; a weight row whose float64 sum differs from
 *                         1 by more than 1e-3; rest normals for a mesh without vertex normals, or none for a mesh with them;
 *                         posing a shape that has no skin; a shape listed twice; and what a deform batch refuses
 *                         (n_renders == 0, BF_FLAG_ROLLING, a multi-pixel film, a bad to_world)
 *     BF_ERR_UNSUPPORTED  a mesh that carries an emitter / transmitter */
bf_status bf_scene_set_skin(bf_scene *scene, uint32_t shape, uint32_t n_bones, const float *rest_positions /* host [n_vertices][3] */,
                            const float *rest_normals /* host [n_vertices][3] or NULL */, const uint32_t *bone_index /* host [n_vertices][4] */,
                            const float *bone_weight /* host [n_vertices][4] */);
bf_status bf_scene_pose_skin(bf_scene *scene, uint32_t shape, const float *bones /* host [n_bones][12] */, void *stream);
bf_status bf_render_skin_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds,
                                      uint32_t n_skinned, const uint32_t *shapes, const float *const *bones /* [n_skinned] host pointers */,
                                      uint32_t n_shapes, const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream,
                                      bf_stats *stats_out);
bf_status bf_render_skin_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_skinned,
                               const uint32_t *shapes, const float *const *bones, uint32_t n_shapes, const float *to_world, float *hist_out,
                               bf_path_record *records_out, bf_stats *stats_out);

/* Dual-quaternion skinning (Kavan et al.): a skin MODE per handle and mesh shape.  Linear blending averages matrices, so a joint
 * that twists loses volume (its cross-section is halved at 120 degrees of twist and gone at 180); blending unit dual quaternions
 * keeps every vertex at its rest distance from the twist axis.  Storage, bone tables, batches and sweeps are the skin's: only the
 * blend differs, and callers pass the same [n_bones][3][4] tables.  DESIGN.md 6d.
 *   bf_scene_set_skin_mode: BF_SKIN_LINEAR (the default) or BF_SKIN_DUAL_QUATERNION for mesh shape `shape` of this handle.  It
 *     needs a mesh, not a skin, and outlives bf_scene_set_skin; a clone inherits the source's modes when it is taken and owns them
 *     from then on.  Setting it moves nothing: every call that takes bones reads the mode of each skinned shape it poses
 *     (bf_scene_pose_skin, bf_scene_pose_morph with bones, bf_render_skin_batch(_device), bf_render_morph_batch(_device) with bones).
 *   Bones in this mode must be rigid: evaluated in float64, max |R^T R - I| <= 1e-4 and det R > 0.  Anything else is refused with
 *     BF_ERR_INVALID naming the bone, before anything is enqueued; the scene and an open rolling sequence stay as they were.  A
 *     bone that no vertex weighs is checked for finite entries only and enters the table as the identity (1, 0, 0, 0; 0, 0, 0, 0).
 *   bf_bone_dual_quaternions: the conversion the library applies to a bone table, on the host (no device, no scene).  float64,
 *     rounded to float once at the end.  R becomes a quaternion by Shepperd's method: of (trace, m00, m11, m22) the largest, the
 *     first among equals in that order, names the component computed as half a square root (and so positive), the other three are
 *     the matching off-diagonal sums or differences divided by four times it; the quaternion q is then divided by its norm.  The
 *     dual part is (0, t) q / 2.  out = (w, x, y, z) of q, then (w, x, y, z) of the dual part.  EVERY bone must be rigid here.
 *     beifong_amd.motion.bone_dual_quaternions is the numpy restatement, bit for bit.
 *   The blend, fp32, every operation rounded (no FMA, IEEE division and square root).  For a vertex with slots k = 0..3, weights
 *     w_k and the dual quaternions D_k of its bones:
 *       p   = the slot of largest weight, the first among equals;   s_k = -1 if dot(D_k.real, D_p.real) < 0, else +1
 *       b   = ((s0 w0 D_0 + s1 w1 D_1) + s2 w2 D_2) + s3 w3 D_3     per component over all eight, all four terms always evaluated
 *       r   = b.real / |b.real|,  e = b.dual / |b.real|             (dot and |.|^2 are ((a0 b0 + a1 b1) + a2 b2) + a3 b3)
 *       rotate(r, v) = (v + rw t) + cross(r.xyz, t)  with  t = 2 cross(r.xyz, v),   cross(a, b).x = fl(fl(ay bz) - fl(az by))
 *       x'  = rotate(r, x) + 2 ((rw e.xyz - ew r.xyz) + cross(r.xyz, e.xyz))
 *       n'  = rotate(r, n)                                          no translation, not renormalised
 *     beifong_amd.motion.apply_skin_dq is the numpy statement; a morph ahead of the skin feeds (x, n) as in linear mode, and
 *     BF_NORMALS_RECOMPUTE replaces n' as it replaces the linear blend's.
 *   Bound: |x'| <= |X|_2 + W T / kappa per coordinate with the roundings accounted for: X the extent of what is posed, W the
 *     largest weight-row sum, T the largest |t|_2 over the bones some vertex weighs, kappa the smallest over the vertices of the
 *     row's largest weight (|b.real| >= kappa).  The gather's check stays as the safety net.
 *   Refusals: BF_ERR_INVALID for a NULL argument, a shape out of range or not a mesh, an unknown mode; BF_ERR_UNSUPPORTED for
 *     setting the mode of a mesh that carries an emitter / transmitter. */
enum { BF_SKIN_LINEAR = 0, BF_SKIN_DUAL_QUATERNION = 1 };
bf_status bf_scene_set_skin_mode(bf_scene *scene, uint32_t shape, uint32_t mode);
bf_status bf_scene_get_skin_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out);
bf_status bf_bone_dual_quaternions(uint32_t n_bones, const float *bones /* host [n_bones][12] */, float *out /* host [n_bones][8] */);

/* Morph targets (blend shapes): the moved vertices are a rest shape plus a weighted sum of per-vertex displacement fields,
 * evaluated on the device AHEAD of the skin, as glTF-style pipelines order the two.  A morph is attached to a mesh shape once
 * (rest positions, rest normals for a mesh with vertex normals, n_targets <= 256 dense position deltas [n_targets][n_vertices][3]
 * and optionally normal deltas of the same shape); after that a pose is n_targets weights, any finite floats (negative weights
 * and weights above 1 are legal).  DESIGN.md 6d.
 *   Arithmetic, fp32, every product and sum rounded (no FMA).  For a vertex with rest position r and deltas d_k:
 *       p = r;  for k = 0 .. n_targets-1 in increasing k:  p_c = fl(p_c + fl(w_k d_k,c))                  per coordinate
 *       n likewise from the rest normal and the normal deltas, not renormalised
 *     Every target is always evaluated: a zero weight takes no shortcut, so a -0.0 may come out as +0.0.  With no normal deltas
 *     n is the rest normal copied bit for bit.  If the call also gives bones, the shape must carry a skin (bf_scene_set_skin) and
 *     the result is the skin's arithmetic (above) applied to (p, n) in place of the skin's own rest arrays: its indices and
 *     weights are used, its rest arrays are not read.  Under BF_NORMALS_RECOMPUTE (bf_scene_set_normal_mode) neither morph
 *     normals nor skin normals are computed: the shape gets bf_vertex_normals of the final positions, as after a skin pose.
 *     beifong_amd.motion.apply_morph is the numpy statement; the composition is apply_skin(*apply_morph(...), index, weight, bones).
 *   bf_scene_set_morph: host arrays, deep-copied into one immutable device block.  One morph per shape; a second call replaces
 *     this handle's, n_targets == 0 removes it (the arrays are then not read).  rest_normals: given exactly if the mesh was created
 *     with vertex normals; delta_normals: NULL, or given together with rest_normals.  Clones taken afterwards share the block; a
 *     later call on either handle changes that handle alone.  The mesh itself does not move.  bf_scene_rebuild_bvh keeps morphs.
 *   bf_scene_pose_morph: bf_scene_pose_skin's semantics word for word: the mesh's BASE becomes the computed vertices, whatever it
 *     held before; the handle's pose goes on top; an open rolling sequence is finished first; ordering and copy on write are
 *     unchanged.  bones: NULL, or the host bone table of the shape's skin.  After the call every path and every bf_ray_intersect /
 *     bf_trace_* result is bit-identical to a bf_scene_create of the description with the shape carrying the numpy statement's
 *     arrays, followed by the same transform call.  weights and bones are free again when the call returns.
 *   bf_render_morph_batch(_device): bf_render_skin_batch with weights[j] = host [n_renders][n_targets(shapes[j])] and bones
 *     either NULL (no shape is skinned) or [n_morphed] host pointers, entry j NULL (shape j is morphed only) or
 *     [n_renders][n_bones(shapes[j])][12].  Render k is bit-identical to bf_scene_pose_morph(slice k) +
 *     bf_scene_transform_meshes(to_world[k]) + a stand-alone render with seeds[k] on a second handle.  Arena, chunking
 *     (BF_MOTION_BATCH_MB) and launch flags as a skin batch; the handle's base, pose and clones do not change.
 *   Scratch: the posed vertices go to the skin's posed-vertex buffer, under its sizing rules, OUTSIDE BF_MOTION_BATCH_MB.
 *   Bound: derived on the host, per axis max |rest| + sum_k |w_k| max |d_k| with the roundings accounted for; with bones it is
 *     fed through the skin bound in place of the skin's rest extent.  A zero weight keeps its target out of the bound however
 *     large its deltas.  A bound float cannot hold is refused; the gather's check stays as the safety net.
 *   Validation, before anything is enqueued (a failed call leaves the scene as it was; the text names shape, vertex, target or bone):
 *     BF_ERR_INVALID      a shape index out of range or not a mesh; NULL arrays; n_targets > 256; a non-finite rest, delta,
 *                         weight or bone value; rest normals for a mesh without vertex normals, or none for a mesh with them;
 *                         normal deltas without rest normals; posing a shape that has no morph; bones for a shape that has no
 *                         skin; a shape listed twice; and what a skin batch refuses (n_renders == 0, BF_FLAG_ROLLING, a
 *                         multi-pixel film, a bad to_world)
 *     BF_ERR_UNSUPPORTED  a mesh that carries an emitter / transmitter
 *     BF_ERR_NOMEM        the device block cannot be allocated */
bf_status bf_scene_set_morph(bf_scene *scene, uint32_t shape, uint32_t n_targets, const float *rest_positions /* host [n_vertices][3] */,
                             const float *rest_normals /* host [n_vertices][3] or NULL */,
                             const float *delta_positions /* host [n_targets][n_vertices][3] */,
                             const float *delta_normals /* host [n_targets][n_vertices][3] or NULL */);
bf_status bf_scene_pose_morph(bf_scene *scene, uint32_t shape, const float *weights /* host [n_targets] */,
                              const float *bones /* host [n_bones][12] or NULL */, void *stream);
bf_status bf_render_morph_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds,
                                       uint32_t n_morphed, const uint32_t *shapes, const float *const *weights /* [n_morphed] host pointers */,
                                       const float *const *bones /* NULL, or [n_morphed] host pointers (entries may be NULL) */,
                                       uint32_t n_shapes, const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream,
                                       bf_stats *stats_out);
bf_status bf_render_morph_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_morphed,
                                const uint32_t *shapes, const float *const *weights, const float *const *bones, uint32_t n_shapes,
                                const float *to_world, float *hist_out, bf_path_record *records_out, bf_stats *stats_out);

/* Recomputed vertex normals: angle-weighted face normals, computed on the device wherever a mesh's base positions are
 * replaced, so that a smooth-shaded mesh that deforms or is skinned needs no normal array per frame.  DESIGN.md 6d.
 *   Arithmetic, fp32, every product, sum, difference, quotient and square root rounded (IEEE division and square root), no
 *   FMA outside the engine's fp32 arc cosine (bf_device_math.h, as bf_eval_elementary evaluates it).  For each face f with corners p0, p1, p2:
 *       n  = cross(p1 - p0, p2 - p0), each component fl(fl(a b) - fl(c d));   l2 = fl(fl(fl(nx^2) + fl(ny^2)) + fl(nz^2))
 *       the face contributes nothing unless l2 > 0;   nh = n / sqrt(l2) per component
 *       at corner j:  a = p[j+1] - p[j], b = p[j+2] - p[j], la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)), dot = (x + y) + z of
 *         the rounded products; the corner contributes nothing unless la > 0 and lb > 0 (an edge whose squared length underflows
 *         to zero while l2 > 0); c = dot(a / la, b / lb) clamped to [-1, 1]; theta = that arc cosine of c; contribution fl(nh theta)
 *     and for each vertex: s = +0, plus its contributions IN INCREASING FACE INDEX (one add per component each);
 *     len = sqrt(dot(s, s)); the normal is s / len if len != 0, else (1, 0, 0): a vertex of no face, or of degenerate faces only.
 *   bf_vertex_normals: that statement on the host, bit for bit what the device computes.  It needs no device and no scene: it
 *     is what a caller puts into a description so that frame 0 matches the frames the device recomputes.  BF_ERR_INVALID for a
 *     NULL array (with a non-zero count) or an index >= n_vertices.  beifong_amd.motion.vertex_normals_f32 is its Python face.
 *   bf_scene_set_normal_mode: per handle and mesh shape.  BF_NORMALS_GIVEN (the default): normals are replaced when a call
 *     gives them, kept when not, never recomputed.  BF_NORMALS_RECOMPUTE: wherever the shape's base positions are replaced and
 *     the call carries no normals for it, its base normals become the statement above of the new base positions —
 *     bf_scene_update_vertices(_device), bf_scene_pose_skin (the skin's blended normals are then not computed),
 *     bf_render_deform_batch(_device) for a listed shape whose normals entry is NULL, bf_render_skin_batch(_device).  Explicit
 *     normals in a call win for that call.  In a batch the normals of version k are those of its UNTRANSFORMED positions;
 *     to_world[k] then turns them as it turns given ones (n' = R n, not renormalised).
 *     Contract: after such a call every path and every bf_ray_intersect / bf_trace_* result is bit-identical to a
 *     bf_scene_create of the description with the shape carrying `positions` and bf_vertex_normals(positions), followed by the
 *     same transform call.  Setting the mode changes nothing until the next position update; switching back to GIVEN keeps the
 *     normals last computed.  A clone inherits the source's modes when it is taken and owns them from then on.
 *     The device forms' bound contract is unchanged: a normal that is not finite is refused by the gather and counted like a
 *     given one (the host form of an update under RECOMPUTE is watched the same way: positions may be finite and their cross
 *     products not).
 *   Cost: the first recomputation of a shape builds its inverted index on the host (per vertex, its incident corners in face
 *     order: 48 bytes per face + 4 per vertex on the device), shared by clones and kept across bf_scene_rebuild_bvh.  The
 *     normals are written to a scratch buffer of the handle's own before the gather reads them, 12 bytes per vertex and
 *     version over the recomputing shapes of the call and the renders of the largest chunk; it grows only, is freed with the
 *     handle and lies OUTSIDE the BF_MOTION_BATCH_MB budget, as the skin scratch.
 *   Refusals, nothing enqueued and the scene as it was: BF_ERR_INVALID for a NULL scene, a shape out of range or not a mesh,
 *     an unknown mode, a mesh created without vertex normals; BF_ERR_UNSUPPORTED for a mesh that carries an emitter /
 *     transmitter.  bf_scene_get_normal_mode: BF_ERR_INVALID for a NULL argument, a shape out of range or not a mesh. */
enum { BF_NORMALS_GIVEN = 0, BF_NORMALS_RECOMPUTE = 1 };
bf_status bf_vertex_normals(uint32_t n_vertices, const float *positions /* host [n_vertices][3] */, uint32_t n_faces,
                            const uint32_t *indices /* host [n_faces][3] */, float *normals_out /* host [n_vertices][3] */);
bf_status bf_scene_set_normal_mode(bf_scene *scene, uint32_t shape, uint32_t mode);
bf_status bf_scene_get_normal_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out);

/* Scene::ray_intersect / ray_test over a batch of HOST rays (tests, tools).
 * rays: [n][8] = o.xyz, mint, d.xyz, maxt.  Outputs may be NULL.
 * out_t = +inf on miss; out_prim = global primitive index (shape prefix sum,
 * kdtree.h:2335-2355); out_uv = prim_uv. */
bf_status bf_trace_closest(const bf_scene *scene, uint64_t n, const float *rays,
                           float *out_t, uint32_t *out_prim, uint32_t *out_shape,
                           float *out_uv);
bf_status bf_trace_any(const bf_scene *scene, uint64_t n, const float *rays,
                       uint8_t *out_hit);

/* Scene::ray_intersect returning the whole SurfaceInteraction3f
 * (scene.cpp:129-146 -> PreliminaryIntersection::compute_surface_interaction,
 * interaction.h:613-644; Mesh::compute_surface_interaction mesh.cpp:452-548;
 * Rectangle::compute_surface_interaction rectangle.cpp:265-298).
 * out_si: [n][BF_SI_FLOATS] = t, p.xyz, n.xyz, sh_frame.n.xyz, sh_frame.s.xyz,
 * sh_frame.t.xyz, wi.xyz (local), prim_uv.xy, dp_du.xyz, dp_dv.xyz.
 * A miss has t = +inf and zeros elsewhere.  out_prim / out_shape may be NULL. */
#define BF_SI_FLOATS 27
bf_status bf_ray_intersect(const bf_scene *scene, uint64_t n, const float *rays,
                           float *out_si, uint32_t *out_prim, uint32_t *out_shape);

/* Evaluate the engine's fp32 elementary functions ON THE DEVICE over a HOST
 * array (conformance checks: the kernels use these in place of the libm calls
 * the reference's scalar variants make, e.g. spot.cpp:136, microfacet.h:160-190,
 * wignertransmitter.cpp signal models).  op: 0 sin, 1 cos, 2 acos, 3 exp, 4 log,
 * 5 erf, 6 tan.  Needs no scene. */
bf_status bf_eval_elementary(int op, uint64_t n, const float *x, float *y);

/* The exact accumulator of BF_FLAG_EXACT_SUM on caller-given addends (conformance checks; needs no scene).  Host arrays:
 * out[c] = fl(sum of value[i] over cell[i] == c), the exact sum rounded once to fp32 (nearest-even; subnormals kept; +-inf from
 * 2^128 - 2^103 on), and +0.0 for a cell without addends.
 *   bf_exact_sum_host  the accumulator's arithmetic (csrc/bf_sum.h) on the CPU; needs no device.
 *   bf_exact_sum       on the device, through the device functions the exact-sum render kernels add with and their resolve kernel:
 *                      a grid-stride launch over the addends.  in_lds != 0: the workgroups privatise the cells in LDS and flush
 *                      limbs, where n_cells cells fit the 48 KiB a render privatises in (682); otherwise, and with in_lds = 0,
 *                      every addend goes to the global limbs.  Synchronous.
 * BF_ERR_INVALID for a null pointer (n_cells = 0 included), a cell index that is not below n_cells, a non-finite value, or
 * n >= 2^31 (the limbs' headroom). */
bf_status bf_exact_sum_host(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, float *out);
bf_status bf_exact_sum(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, uint32_t in_lds, float *out);

/* ---------------- plugin-level queries on the device ------------------------------------------------------------------
 * The BSDF, emitter and sensor functions the render kernels call, one query per lane, general kernels (every material,
 * emitter and sensor type; never the lean profile, never BF_FLAG_FAST).  Every path-level result of a render is built from
 * exactly these values, so each query is bit-identical to the oracle's function of the same name (tests/test_gpu_queries.py).
 *
 * Two forms each, like bf_render / bf_render_device:
 *   host form      host arrays, synchronous: stages the rows, runs the _device form on the null stream, copies back and
 *                  waits for that stream
 *   _device form   device pointers (e.g. torch tensors' data_ptr()) and a hipStream_t (NULL = default stream); asynchronous
 *
 * What a query sees: the scene as the handle's next render would — after a preceding bf_scene_update_endpoints or
 *   bf_scene_transform_meshes / bf_scene_translate_meshes on the same stream, the tables a joined endpoint update moved into
 *   the rolling pool included.  Never the geometry versions of a motion batch (bf_render_motion_batch_device).
 * Ordering: like a render, a query waits for the handle's previous work when it is issued on another stream, and the
 *   handle's next call waits for the query, so a later update cannot overwrite a table a query is still reading.  One host
 *   thread at a time per handle (BF_ERR_INVALID otherwise).
 * Rolling sequences: queries only read the scene.  A query issued between two rolling renders leaves the sequence open and
 *   its histograms unchanged.
 * Refusals, before anything is enqueued (a refused call changes nothing):
 *   BF_ERR_INVALID      a null scene; a null pointer with n > 0; n > 2^32 - 1; an emitter index out of range; a material
 *                       index out of range (host forms: checked on the host; the _device forms cannot see the indices and
 *                       write NaN to the rows of out-of-range ones); a bf_eval_microfacet op or distribution out of range
 *   BF_ERR_UNSUPPORTED  transmitter-type emitters (BF_TRANSMITTER_*) and receiver-type sensors (BF_RECEIVER_*): no probe
 *   n == 0 returns BF_OK and launches nothing.
 * Directions of the BSDF queries are in the local shading frame, as si.wi is in BSDF::eval(ctx, si, wo). */

/* BSDF::eval and BSDF::pdf (diffuse.cpp:78-135, roughconductor.cpp:145-392, twosided.cpp:62-180; eval includes the cosine
 * foreshortening).  materials[n]: index into the scene's material table (the twosided back material is selected for
 * wi.z < 0 as the renders do); wi_wo[n][6] = wi.xyz, wo.xyz; out[n][2] = eval, pdf. */
bf_status bf_bsdf_eval_pdf(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_wo, float *out);
bf_status bf_bsdf_eval_pdf_device(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_wo, float *out,
                                  void *stream);

/* BSDF::sample (diffuse.cpp:78-100, roughconductor.cpp:145-218, twosided.cpp:94-130).  wi_u[n][6] = wi.xyz, sample1,
 * sample2.xy (sample1 is unused by these single-lobe BSDFs); out[n][5] = wo.xyz, pdf, weight (eval / pdf). */
bf_status bf_bsdf_sample(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_u, float *out);
bf_status bf_bsdf_sample_device(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_u, float *out,
                                void *stream);

/* Emitter::sample_direction of emitter `emitter` (spot.cpp:97-164, point.cpp:78-103, area.cpp:76-120 -> shape.cpp:323-356).
 * in[n][5] = ref_p.xyz, sample.xy; out[n][8] = d.xyz, dist, pdf, delta (0 / 1), grey spectrum (weight), pdf_direction of the
 * sampled point (area.cpp:122-150; 0 for the delta emitters). */
bf_status bf_emitter_sample_direction(const bf_scene *scene, uint32_t emitter, uint64_t n, const float *in, float *out);
bf_status bf_emitter_sample_direction_device(const bf_scene *scene, uint32_t emitter, uint64_t n, const float *in, float *out,
                                             void *stream);

/* Sensor::sample_ray of the scene's sensor (perspective.cpp:172-199, fluxmeter.cpp:63-85, irradiancemeter.cpp:63-85,
 * radiancemeter.cpp:91-108).  in[n][4] = film position.xy in [0, 1]^2 of the crop window, aperture sample.xy; out[n][9] =
 * o.xyz, mint, d.xyz, ray weight, maxt.  Time and wavelength samples are not read by these sensors. */
bf_status bf_sensor_sample_ray(const bf_scene *scene, uint64_t n, const float *in, float *out);
bf_status bf_sensor_sample_ray_device(const bf_scene *scene, uint64_t n, const float *in, float *out, void *stream);

/* Scene::ray_intersect / ray_test on DEVICE rays [n][8], stream-ordered: the kernel of bf_ray_intersect / bf_trace_any,
 * so the results are bit-identical to theirs.  out_si[n][BF_SI_FLOATS] (required), out_prim / out_shape may be NULL;
 * out_hit[n] = 0 / 1. */
bf_status bf_ray_intersect_device(const bf_scene *scene, uint64_t n, const float *rays, float *out_si, uint32_t *out_prim,
                                  uint32_t *out_shape, void *stream);
bf_status bf_trace_any_device(const bf_scene *scene, uint64_t n, const float *rays, uint8_t *out_hit, void *stream);

/* MicrofacetDistribution on the device (include/mitsuba/render/microfacet.h:60-400; the golden vectors of
 * src/librender/tests/test_microfacet.py).  Needs no scene.  distribution: BF_MF_*; in[n][8] = wi.xyz, m.xyz, s.xy;
 * op 0: out[i][0] = eval(m); 1: pdf(wi, m); 2: smith_g1(v = m, m = wi); 3: sample(wi, s) -> out[i] = m.xyz, pdf.
 * Ops 0-2 write 0 to out[i][1..3]. */
bf_status bf_eval_microfacet(int op, uint32_t distribution, float alpha_u, float alpha_v, uint32_t sample_visible, uint64_t n,
                             const float *in, float *out);

#ifdef __cplusplus
}
#endif
#endif /* BEIFONG_HIP_H */
