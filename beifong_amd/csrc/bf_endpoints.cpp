// The endpoint tables behind bf_scene_create / bf_scene_update_endpoints / bf_scene_clone / bf_scene_set_classes (include/beifong_hip.h):
// a description's rectangles, shapes, emitters, materials and sensor flattened into one host image, the profile derived from it, the
// one device block the kernels read it from and its versions within a rolling sequence.  State: bf_scene::ends (bf_scene.h: EndpointState).
#include "bf_scene.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

namespace {
void m34(const float *m16, float *out12) { std::memcpy(out12, m16, 12 * sizeof(float)); }

inline float fmaf_(float a, float b, float c) { return std::fmaf(a, b, c); }
struct V3 {
    float x, y, z;
};
// same conventions as the device code (bf_device_math.h)
inline V3 xf_vector(const float *m, V3 v) {
    V3 r = {m[0] * v.x, m[4] * v.x, m[8] * v.x};
    r = {fmaf_(m[1], v.y, r.x), fmaf_(m[5], v.y, r.y), fmaf_(m[9], v.y, r.z)};
    r = {fmaf_(m[2], v.z, r.x), fmaf_(m[6], v.z, r.y), fmaf_(m[10], v.z, r.z)};
    return r;
}
inline float dot(V3 a, V3 b) { return fmaf_(a.z, b.z, fmaf_(a.y, b.y, a.x * b.x)); }
inline V3 cross(V3 a, V3 b) {
    return {fmaf_(a.y, b.z, -(a.z * b.y)), fmaf_(a.z, b.x, -(a.x * b.z)), fmaf_(a.x, b.y, -(a.y * b.x))};
}
inline V3 normalize(V3 a) {
    float s = 1.f / std::sqrt(dot(a, a));
    return {a.x * s, a.y * s, a.z * s};
}

bool any_resample_of(const std::vector<bfd::DEmitter> &emitters) {
    for (const auto &e : emitters)
        if (e.resample != 0u) return true;
    return false;
}

void set_classes_ptr(bfd::DScene &d, const uint32_t *p) {
    d.class_lo = (uint32_t) (uintptr_t) p;
    d.class_hi = (uint32_t) ((uint64_t) (uintptr_t) p >> 32);
}
// words of the handle's class array: shape_class[n_shapes], the arrival table (bf_arrival.h) or the range-rate table's header and rows
// (bf_range_rate.h), whichever form is installed
size_t class_words(uint32_t n_shapes) { return std::max<size_t>(bfa::kWords, (size_t) bfr::table_words(n_shapes)); }

// what bf_scene_create and bf_scene_update_endpoints both require of the material table and the film (a back_material out of
// range would send the kernels' load_material past the device table)
bf_status check_materials_and_film(const bf_scene_desc *desc) {
    if (desc->n_materials == 0 || !desc->materials) return fail(BF_ERR_INVALID, "at least one material is required");
    for (uint32_t i = 0; i < desc->n_materials; ++i) {
        const uint32_t b = desc->materials[i].back_material;
        if (b == 0) continue;
        if (b > desc->n_materials || !desc->materials[i].twosided || !desc->materials[b - 1].twosided || desc->materials[b - 1].back_material != 0)
            return fail(BF_ERR_INVALID, "material %u: back_material %u must name a twosided table entry without a back side of its own", i, b);
    }
    if (desc->sensor.film_width == 0 || desc->sensor.film_height == 0)
        return fail(BF_ERR_INVALID, "sensor film is %u x %u", desc->sensor.film_width, desc->sensor.film_height);
    return BF_OK;
}

// a small host table into the handle's device array `dst` in stream order, through the scene's pinned staging ring: the caller's
// table is free again when the call returns
bf_status stage_copy(const bf_scene *sc, void *dst, const void *src, size_t bytes, hipStream_t stream) {
    bf_scene::Stage *stg = nullptr;
    bf_status st = stage_acquire(sc, bytes, &stg);
    if (st != BF_OK) return st;
    std::memcpy(stg->host, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst, stg->host, bytes, hipMemcpyHostToDevice, stream));
    return stage_release_after(stg, stream);
}

// the spare words of a range-rate table (bf_range_rate.h) from the handle's velocity modes (bf_velocity.h): every shape's mode behind its
// `lin`, the address `rows` of the velocity rows in the header; without rows every shape reads as BF_VELOCITY_TWIST
void velocity_patch(const bf_scene *scene, std::vector<uint32_t> &words, const float4 *rows) {
    const uint32_t n_shapes = scene->ends.n_shapes;
    if (words.size() != (size_t) bfr::table_words(n_shapes)) return;
    words[6] = (uint32_t) (uintptr_t) rows;
    words[7] = (uint32_t) ((uint64_t) (uintptr_t) rows >> 32);
    static_assert(offsetof(bfr::Header, pad) == 24 && offsetof(bfr::Row, pad0) == 12, "the spare words of the range-rate table");
    for (uint32_t k = 0; k < n_shapes; ++k) words[bfr::kHeaderWords + (size_t) bfr::kRowWords * k + 3] = rows ? scene->mesh.velocity_mode(k) : 0u;
}

// what bf_scene_set_classes, bf_scene_set_arrival_classes and bf_scene_set_range_rate_classes share: the open rolling sequence ends (its renders were issued without
// classes; the table is not theirs to see change), the handle's device array exists, `words` go into it in stream order
bf_status install_classes(bf_scene *scene, const void *words, size_t bytes, uint32_t class_info, hipStream_t stream) {
    bf_status st = order_after_last(scene, stream);
    if (st == BF_OK) st = close_sequence(scene, stream);
    if (st != BF_OK) return st;
    if (!(class_info & bfd::kClassRangeRate)) scene->ends.rr_words.clear();
    if (!class_info) {
        scene->d.class_info = 0u;      // (the device array stays with the handle)
        return BF_OK;
    }
    EndpointState &e = scene->ends;
    if (!e.classes) {
        HIP_TRY(hipMalloc((void **) &e.classes, sizeof(uint32_t) * class_words(e.n_shapes)));
        set_classes_ptr(scene->d, e.classes);
    }
    if (bytes && (st = stage_copy(scene, e.classes, words, bytes, stream)) != BF_OK) return st;
    scene->d.class_info = class_info;
    return mark_last(scene, stream);
}

// Phased-array tables arrive as host pointers inside the flattened records: copy them to the device (allocating on
// scene creation, in place — same sizes required — on bf_scene_update_endpoints: beam steering between frames) and
// patch the records with the device addresses.
bf_status bind_arrays(const bf_scene *sc, EndpointState::Image &f, hipStream_t stream, bool creating) {
    EndpointState &e = sc->ends;
    auto put = [&](const float *host, uint32_t n, float *&dev, uint32_t &dev_n) -> bf_status {
        const size_t bytes = (size_t) n * BF_VELEM_FLOATS * sizeof(float);
        if (!creating) {
            if (!dev || dev_n != n)
                return fail(BF_ERR_INVALID, "bf_scene_update_endpoints: phased array size changed (%u -> %u virtual elements)", dev_n, n);
            return stage_copy(sc, dev, host, bytes, stream);
        }
        HIP_TRY(hipMalloc((void **) &dev, bytes));
        dev_n = n;
        HIP_TRY(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
        return BF_OK;
    };
    if (creating) {
        e.array_dev.assign(f.emitters.size(), nullptr);
        e.array_n.assign(f.emitters.size(), 0u);
    }
    for (size_t i = 0; i < f.emitters.size(); ++i) {
        if (f.emitters[i].type != BF_TRANSMITTER_PHASED) continue;
        if (i >= e.array_dev.size()) return fail(BF_ERR_INVALID, "emitter layout changed");
        bf_status st = put(f.emitters[i].velems, f.emitters[i].n_velems, e.array_dev[i], e.array_n[i]);
        if (st != BF_OK) return st;
        f.emitters[i].velems = e.array_dev[i];
    }
    if (f.sensor.type == BF_RECEIVER_PHASED) {
        bf_status st = put(f.sensor.velems, f.sensor.n_velems, e.sensor_array_dev, e.sensor_array_n);
        if (st != BF_OK) return st;
        f.sensor.velems = e.sensor_array_dev;
    }
    return BF_OK;
}

// `bytes` of device memory at `from` in an allocation of the caller's own (nothing, *to = nullptr, if there is none)
template <class T> bf_status dup(const T *from, size_t bytes, T **to) {
    *to = nullptr;
    if (!from || !bytes) return BF_OK;
    HIP_TRY(hipMalloc((void **) to, bytes));
    HIP_TRY(hipMemcpy(*to, from, bytes, hipMemcpyDeviceToDevice));
    return BF_OK;
}
}  // namespace

// ---- EndpointState (bf_scene.h) ----
void EndpointState::apply(const Image &img, bool tab_cache) {
    n_rects = d->n_rects = (uint32_t) img.rects.size();
    n_shapes = (uint32_t) img.shapes.size();
    n_emitters = d->n_emitters = (uint32_t) img.emitters.size();
    n_materials = d->n_materials = (uint32_t) img.materials.size();
    d->tab_cache = (tab_cache && n_materials <= bfd::kTabMaxMaterials && n_rects <= bfd::kTabMaxRects) ? 1u : 0u;
    d->c = img.c;
    d->lambda_min = img.lambda_min;
    d->lambda_max = img.lambda_max;
    emitter_types.clear();
    for (const auto &e : img.emitters) emitter_types.push_back(e.type);
    any_resample = any_resample_of(img.emitters);
    any_back_material = false;      // (lean_profile: the lean kernels have one BSDF per material)
    for (const auto &m : img.materials) any_back_material = any_back_material || m.m.back_material != 0;
    sensor_host = img.sensor;
    film_w = img.film_w;
    film_h = img.film_h;
    adc_t = img.window_t ? img.window_t : img.sensor.t_bins;
    adc_f = img.window_f ? img.window_f : img.sensor.f_bins;
    auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    lay.o_rects = 0;
    lay.o_shapes = lay.o_rects + up16(n_rects * sizeof(bfd::DRect));
    lay.o_emit = lay.o_shapes + up16(n_shapes * sizeof(bfd::DShape));
    lay.o_mat = lay.o_emit + up16(n_emitters * sizeof(bfd::DEmitter));
    lay.o_sensor = lay.o_mat + up16(n_materials * sizeof(bfd::DMaterial));
    lay.total = lay.o_sensor + up16(sizeof(bfd::DSensor));
}
void EndpointState::pack(const Image &img, char *blk) const {
    if (n_rects) std::memcpy(blk + lay.o_rects, img.rects.data(), n_rects * sizeof(bfd::DRect));
    if (n_shapes) std::memcpy(blk + lay.o_shapes, img.shapes.data(), n_shapes * sizeof(bfd::DShape));
    if (n_emitters) std::memcpy(blk + lay.o_emit, img.emitters.data(), n_emitters * sizeof(bfd::DEmitter));
    if (n_materials) std::memcpy(blk + lay.o_mat, img.materials.data(), n_materials * sizeof(bfd::DMaterial));
    std::memcpy(blk + lay.o_sensor, &img.sensor, sizeof(bfd::DSensor));
}
void EndpointState::point_at(const char *blk) {
    d->rects = n_rects ? (const bfd::DRect *) (blk + lay.o_rects) : nullptr;
    d->shapes = n_shapes ? (const bfd::DShape *) (blk + lay.o_shapes) : nullptr;
    d->emitters = n_emitters ? (const bfd::DEmitter *) (blk + lay.o_emit) : nullptr;
    d->materials = n_materials ? (const bfd::DMaterial *) (blk + lay.o_mat) : nullptr;
    d->sensor = (const bfd::DSensor *) (blk + lay.o_sensor);
}
bf_status EndpointState::claim(char **blk) {
    if (!pool) {
        stride = (lay.total + 255) & ~size_t(255);
        HIP_TRY(hipMalloc((void **) &pool, stride * bfd::kRollRing));
    }
    *blk = pool + stride * next;
    return BF_OK;
}
bf_status EndpointState::go_home(hipStream_t stream) {
    if (!in_pool) return BF_OK;
    // The block is found from the sensor record, the one table every update repoints (d->rects stays null in a scene without
    // rectangles).
    const char *blk = (const char *) d->sensor - lay.o_sensor;
    point_at(home);
    in_pool = false;
    next = 0;
    HIP_TRY(hipMemcpyAsync(home, blk, lay.total, hipMemcpyDeviceToDevice, stream));
    return BF_OK;
}
EndpointState::~EndpointState() {
    if (home) (void) hipFree(home);
    if (pool) (void) hipFree(pool);
    for (float *p : array_dev)
        if (p) (void) hipFree(p);
    if (sensor_array_dev) (void) hipFree(sensor_array_dev);
    if (classes) (void) hipFree(classes);
}

extern "C" {

bf_status endpoints_flatten(const bf_scene_desc *desc, EndpointState::Image &f) {
    if (desc->n_shapes && !desc->shapes) return fail(BF_ERR_INVALID, "shapes is null");
    {
        bf_status mst = check_materials_and_film(desc);
        if (mst != BF_OK) return mst;
    }
    std::vector<bfd::DShape> &shapes = f.shapes;
    std::vector<bfd::DRect> &rects = f.rects;
    uint32_t prim = 0;
    uint64_t n_tris_total = 0;
    for (uint32_t i = 0; i < desc->n_shapes; ++i) {
        const bf_shape &s = desc->shapes[i];
        if (s.material >= desc->n_materials) return fail(BF_ERR_INVALID, "shape %u: material index out of range", i);
        if (s.emitter >= (int32_t) desc->n_emitters) return fail(BF_ERR_INVALID, "shape %u: emitter index out of range", i);
        bfd::DShape ds;
        ds.type = s.type;
        ds.material = s.material;
        ds.emitter = s.emitter;
        ds.rect = -1;
        {
            bool any = false;
            for (int k = 0; k < 16; ++k) any = any || s.velocity[k] != 0.f;
            for (int k = 0; k < 12; ++k) ds.velocity[k] = any ? s.velocity[k] : ((k % 5 == 0) ? 1.f : 0.f);    // all zeros = identity
        }
        if (s.type == BF_SHAPE_RECTANGLE) {
            bfd::DRect rc;
            m34(s.to_world, rc.to_world);
            m34(s.to_object, rc.to_object);
            // Rectangle::update — src/shapes/rectangle.cpp:83-92
            V3 dp_du = xf_vector(rc.to_world, V3{2.f, 0.f, 0.f});
            V3 dp_dv = xf_vector(rc.to_world, V3{0.f, 2.f, 0.f});
            V3 n = normalize(V3{s.to_object[8], s.to_object[9], s.to_object[10]});   // inverse-transpose * (0,0,1)
            rc.s[0] = dp_du.x; rc.s[1] = dp_du.y; rc.s[2] = dp_du.z;
            rc.t[0] = dp_dv.x; rc.t[1] = dp_dv.y; rc.t[2] = dp_dv.z;
            rc.n[0] = n.x; rc.n[1] = n.y; rc.n[2] = n.z;
            V3 c = cross(dp_du, dp_dv);
            float area = std::sqrt(dot(c, c));
            if (!(area > 0.f) || !std::isfinite(area)) return fail(BF_ERR_INVALID, "shape %u: degenerate rectangle", i);
            rc.inv_area = 1.f / area;
            rc.area = area;
            rc.shape = i;
            rc.prim = prim;
            rc.material = s.material;
            rc.emitter = s.emitter;
            ds.rect = (int32_t) rects.size();
            rects.push_back(rc);
            prim += 1;
        } else if (s.type == BF_SHAPE_MESH) {
            if (s.n_faces && (!s.positions || !s.indices)) return fail(BF_ERR_INVALID, "shape %u: null mesh arrays", i);
            n_tris_total += s.n_faces;      // (the triangles themselves: bf_api.cpp, gather_triangles)
            prim += s.n_faces;
        } else {
            return fail(BF_ERR_UNSUPPORTED, "shape %u: unknown type %u", i, s.type);
        }
        shapes.push_back(ds);
    }
    if (n_tris_total >= (1u << 28)) return fail(BF_ERR_UNSUPPORTED, "too many triangles");
    f.n_tris = (uint32_t) n_tris_total;

    std::vector<bfd::DEmitter> &emitters = f.emitters;
    for (uint32_t i = 0; i < desc->n_emitters; ++i) {
        const bf_emitter &e = desc->emitters[i];
        bfd::DEmitter de;
        std::memset(&de, 0, sizeof(de));
        de.type = e.type;
        de.rect = -1;
        de.radiance = e.radiance;
        if (e.type == BF_EMITTER_POINT) {
            m34(e.to_world, de.to_world);
        } else if (e.type == BF_EMITTER_SPOT) {
            m34(e.to_world, de.to_world);
            m34(e.to_object, de.to_object);
            // SpotLight ctor — src/emitters/spot.cpp:83-93
            const float pi = 3.14159265358979323846f;
            de.cutoff = e.cutoff_angle_deg * (pi / 180.f);
            de.beam = e.beam_width_deg * (pi / 180.f);
            de.inv_transition = 1.0f / (de.cutoff - de.beam);
            de.cos_cutoff = bfk_host_cos(de.cutoff);
            de.cos_beam = bfk_host_cos(de.beam);
        } else if (e.type == BF_EMITTER_AREA || e.type == BF_TRANSMITTER_AREA || e.type == BF_TRANSMITTER_WIGNER ||
                   e.type == BF_TRANSMITTER_PHASED) {
            if (e.shape < 0 || e.shape >= (int32_t) desc->n_shapes || desc->shapes[e.shape].type != BF_SHAPE_RECTANGLE)
                return fail(BF_ERR_UNSUPPORTED, "emitter %u: area emitters / transmitters must sit on a rectangle", i);
            de.rect = shapes[e.shape].rect;
            if (e.type == BF_TRANSMITTER_PHASED) {
                if (!e.array.velems || e.array.n_velems == 0) return fail(BF_ERR_INVALID, "emitter %u: phased transmitter without array elements", i);
                de.velems = e.array.velems;          // host pointer for now; replaced by the device copy on upload
                de.n_velems = e.array.n_velems;
                for (int k = 0; k < 3; ++k) de.wid[k] = e.array.elem_dims[k];
            }
            if (e.type == BF_TRANSMITTER_WIGNER || e.type == BF_TRANSMITTER_PHASED) {
                if (e.signal_type > BF_SIGNAL_LINFMCW) return fail(BF_ERR_INVALID, "emitter %u: unknown signal type", i);
                // sample_delta_frequency (wignertransmitter.cpp:152-168) defines the frequency for "linfmcw" and "cw" only
                if (e.resample_freq && e.signal_type == BF_SIGNAL_PULSE)
                    return fail(BF_ERR_UNSUPPORTED, "emitter %u: resample_freq=true with signaltype \"pulse\" reads an uninitialised frequency in the "
                                                    "reference (wignertransmitter.cpp:152-168); use \"linfmcw\" or \"cw\"", i);
                de.resample = e.resample_freq ? 1u : 0u;
                de.signal_type = e.signal_type;
                de.amplitude = e.amplitude;
                de.freq_centre = e.freq_centre;
                de.freq_ext = e.freq_ext;
                de.pulse_len = e.pulse_len;
                de.prf = e.prf;
                de.gain = e.gain;
            }
        } else {
            return fail(BF_ERR_UNSUPPORTED, "emitter %u: type %u not supported by this build", i, e.type);
        }
        emitters.push_back(de);
    }

    f.materials.resize(desc->n_materials);      // 48-byte device records (bf_device.h: DMaterial)
    for (uint32_t i = 0; i < desc->n_materials; ++i) {
        f.materials[i].m = desc->materials[i];
        f.materials[i].pad = 0u;
    }

    bfd::DSensor &sen = f.sensor;
    std::memset(&sen, 0, sizeof(sen));
    sen.type = desc->sensor.type;
    sen.rect = -1;
    if (desc->sensor.type == BF_SENSOR_FLUXMETER || desc->sensor.type == BF_SENSOR_IRRADIANCEMETER || desc->sensor.type == BF_RECEIVER_OMNI ||
        desc->sensor.type == BF_RECEIVER_WIGNER || desc->sensor.type == BF_RECEIVER_PHASED) {
        int32_t sh = desc->sensor.shape;
        if (sh < 0 || sh >= (int32_t) desc->n_shapes || desc->shapes[sh].type != BF_SHAPE_RECTANGLE) {
            return fail(BF_ERR_UNSUPPORTED, "fluxmeter / receiver must sit on a rectangle");
        }
        sen.rect = shapes[sh].rect;
        sen.adc_sampling_start = desc->sensor.adc_sampling_start;
        sen.adc_sampling_time = desc->sensor.adc_sampling_time;
        sen.t_bins = desc->sensor.t_bins;
        sen.f_bins = desc->sensor.f_bins;
        sen.t_bandwidth = desc->sensor.t_bandwidth;
        sen.f_bandwidth = desc->sensor.f_bandwidth;
        sen.freq_centre = desc->sensor.freq_centre;
        sen.freq_ext = desc->sensor.freq_ext;
        sen.gain = desc->sensor.gain;
        sen.rx_sig_is_delta = desc->sensor.rx_sig_is_delta;
        if (desc->sensor.rx_signal_type > BF_SIGNAL_LINFMCW) return fail(BF_ERR_INVALID, "sensor: unknown rx_signal_type %u", desc->sensor.rx_signal_type);
        sen.rx_signal = desc->sensor.rx_signal_type;
        sen.rx_pulse_len = desc->sensor.rx_pulse_len;
        sen.rx_prf = desc->sensor.rx_prf;
        sen.rx_amplitude = desc->sensor.rx_amplitude;
        {
            const bf_sensor &ds = desc->sensor;
            if (ds.window_t_bins || ds.window_f_bins || ds.window_offset_t || ds.window_offset_f) {      // adc.cpp:80-91
                if (ds.window_t_bins == 0 || ds.window_f_bins == 0 || (uint64_t) ds.window_offset_t + ds.window_t_bins > ds.t_bins ||
                    (uint64_t) ds.window_offset_f + ds.window_f_bins > ds.f_bins)
                    return fail(BF_ERR_INVALID, "Invalid window specification! offset (%u, %u) + window size (%u, %u) vs full size (%u, %u)",
                                ds.window_offset_t, ds.window_offset_f, ds.window_t_bins, ds.window_f_bins, ds.t_bins, ds.f_bins);
                sen.win_off_t = ds.window_offset_t;
                sen.win_off_f = ds.window_offset_f;
                f.window_t = ds.window_t_bins;
                f.window_f = ds.window_f_bins;
            }
        }
        if (desc->sensor.type == BF_RECEIVER_PHASED) {
            if (!desc->sensor.array.velems || desc->sensor.array.n_velems == 0)
                return fail(BF_ERR_INVALID, "phased receiver without array elements");
            sen.velems = desc->sensor.array.velems;      // host pointer for now (see bind_arrays)
            sen.n_velems = desc->sensor.array.n_velems;
            for (int k = 0; k < 3; ++k) sen.wid[k] = desc->sensor.array.elem_dims[k];
        }
    } else if (desc->sensor.type == BF_SENSOR_RADIANCEMETER) {
        m34(desc->sensor.to_world, sen.to_world);
    } else if (desc->sensor.type == BF_SENSOR_PERSPECTIVE) {
        m34(desc->sensor.to_world, sen.to_world);
        std::memcpy(sen.sample_to_camera, desc->sensor.sample_to_camera, 16 * sizeof(float));
    } else {
        return fail(BF_ERR_UNSUPPORTED, "sensor type %u not supported by this build", desc->sensor.type);
    }
    {
        // ImageBlock::put / SignalBlock::put take the filtered branch iff radius > 0.5 + RayEpsilon (imageblock.cpp:115)
        const bf_rfilter &rf = desc->sensor.rfilter;
        const float ray_eps = 1500.f * 5.9604644775390625e-8f;          // math::RayEpsilon<float> = Epsilon * 1500
        if (!(rf.radius >= 0.f) || !std::isfinite(rf.radius) || rf.radius > 64.f) return fail(BF_ERR_INVALID, "reconstruction filter radius %g", rf.radius);
        if (rf.radius > .5f + ray_eps) {
            sen.filt_n = (uint32_t) std::ceil((rf.radius - 2.f * ray_eps) * 2.f);
            sen.filt_border = rf.border;
            sen.filt_block = rf.block_size;
            sen.filt_radius = rf.radius;
            sen.filt_scale = rf.scale;
            for (int k = 0; k <= BF_FILTER_RESOLUTION; ++k) sen.filt_tab[k] = rf.values[k];
            if (rf.border > 64u || !(rf.scale > 0.f)) return fail(BF_ERR_INVALID, "reconstruction filter: border %u, scale %g", rf.border, rf.scale);
        }
    }
    sen.crop_x = desc->sensor.crop_offset_x;
    sen.crop_y = desc->sensor.crop_offset_y;
    if (sen.crop_x > (1u << 20) || sen.crop_y > (1u << 20)) return fail(BF_ERR_INVALID, "film crop offset (%u, %u) out of range", sen.crop_x, sen.crop_y);
    sen.near_clip = desc->sensor.near_clip;
    sen.far_clip = desc->sensor.far_clip;
    sen.shutter_open = desc->sensor.shutter_open;
    sen.shutter_open_time = desc->sensor.shutter_open_time;
    f.film_w = desc->sensor.film_width;
    f.film_h = desc->sensor.film_height;
    f.c = desc->physics.c;
    f.lambda_min = desc->physics.lambda_min_nm;
    f.lambda_max = desc->physics.lambda_max_nm;

    // rays start on scene surfaces, sensors or emitters: bound |origin| for the builder's padding
    float &origin_scale = f.origin_scale;
    origin_scale = 0.f;
    auto grow_scale = [&](const float *m /* 3x4 */, float ex, float ey) {
        for (int r = 0; r < 3; ++r)
            origin_scale = std::max(origin_scale, std::fabs(m[4 * r + 3]) + std::fabs(m[4 * r + 0]) * ex + std::fabs(m[4 * r + 1]) * ey);
    };
    for (const auto &r : rects) grow_scale(r.to_world, 1.f, 1.f);
    for (const auto &e : emitters) grow_scale(e.to_world, 0.f, 0.f);
    grow_scale(sen.to_world, 0.f, 0.f);
    return BF_OK;
}

bf_status endpoints_create(bf_scene *sc, EndpointState::Image &img, uint64_t *bytes) {
    EndpointState &e = sc->ends;
    e.d = &sc->d;
    bf_status st = bind_arrays(sc, img, nullptr, true);
    if (st != BF_OK) return st;
    e.apply(img, sc->tun.tab_cache);
    e.shapes_host = img.shapes;
    std::vector<char> blk(e.lay.total, 0);
    e.pack(img, blk.data());
    HIP_TRY(hipMalloc((void **) &e.home, e.lay.total));
    HIP_TRY(hipMemcpy(e.home, blk.data(), e.lay.total, hipMemcpyHostToDevice));
    e.point_at(e.home);
    *bytes += e.lay.total;
    return BF_OK;
}

bf_status endpoints_clone(const bf_scene *src, bf_scene *sc) {
    const EndpointState &s = src->ends;
    EndpointState &e = sc->ends;
    e = s;      // the profile, the counts and the layout ... and none of src's allocations: the clone's own copies follow
    e.d = &sc->d;
    e.home = e.pool = nullptr;
    e.next = 0;
    e.in_pool = false;
    e.array_dev.assign(s.array_dev.size(), nullptr);
    e.sensor_array_dev = nullptr;
    e.classes = nullptr;
    bf_status st = dup(s.home, s.lay.total, &e.home);      // (src's sequence is closed: its tables are home)
    if (st != BF_OK) return st;
    e.point_at(e.home);
    // the emitter and sensor records carry device pointers to their phased-array tables: duplicate the tables and re-point the records
    auto repoint = [&](const float *from, uint32_t n, float **to, size_t record) -> bf_status {
        if ((st = dup(from, sizeof(float) * BF_VELEM_FLOATS * n, to)) != BF_OK || !*to) return st;
        HIP_TRY(hipMemcpy(e.home + record, to, sizeof(*to), hipMemcpyHostToDevice));
        return BF_OK;
    };
    for (size_t i = 0; i < s.array_dev.size(); ++i)
        if ((st = repoint(s.array_dev[i], s.array_n[i], &e.array_dev[i], e.lay.o_emit + i * sizeof(bfd::DEmitter) + offsetof(bfd::DEmitter, velems))) != BF_OK)
            return st;
    if ((st = repoint(s.sensor_array_dev, s.sensor_array_n, &e.sensor_array_dev, e.lay.o_sensor + offsetof(bfd::DSensor, velems))) != BF_OK) return st;
    if (e.sensor_array_dev) e.sensor_host.velems = e.sensor_array_dev;
    // the class table (bf_scene_set_classes): the clone's own copy; class_info came with src->d
    if ((st = dup(s.classes, sizeof(uint32_t) * class_words(s.n_shapes), &e.classes)) != BF_OK) return st;
    set_classes_ptr(sc->d, e.classes);
    if (!e.classes) sc->d.class_info = 0u;
    // a range-rate table names the velocity rows it reads: the clone's own (mesh_clone_snapshot has made them)
    if (e.classes && !e.rr_words.empty()) {
        velocity_patch(sc, e.rr_words, sc->mesh.vel);
        HIP_TRY(hipMemcpy(e.classes, e.rr_words.data(), sizeof(uint32_t) * e.rr_words.size(), hipMemcpyHostToDevice));
    }
    return BF_OK;
}

bf_status velocity_stamp(bf_scene *scene, const float4 *rows, hipStream_t stream) {
    EndpointState &e = scene->ends;
    if (!bfd::scene_class_range_rate(scene->d) || e.rr_words.empty() || !e.classes) return BF_OK;
    velocity_patch(scene, e.rr_words, rows);
    return install_classes(scene, e.rr_words.data(), sizeof(uint32_t) * e.rr_words.size(), scene->d.class_info, stream);
}

bf_status bf_scene_update_endpoints(bf_scene *scene, const bf_scene_desc *desc, void *stream_) {
    if (!scene || !desc) return fail(BF_ERR_INVALID, "null argument");
    EndpointState::Image f;
    bf_status st = endpoints_flatten(desc, f);
    if (st != BF_OK) return st;
    EndpointState &e = scene->ends;
    if (f.shapes.size() != e.n_shapes || f.rects.size() != e.n_rects || f.emitters.size() != e.n_emitters || f.n_tris != scene->d.n_tris ||
        f.materials.size() != e.n_materials)
        return fail(BF_ERR_INVALID, "bf_scene_update_endpoints: the description has a different layout than the scene "
                                    "(shapes %zu/%u, rectangles %zu/%u, emitters %zu/%u, triangles %u/%u)",
                    f.shapes.size(), e.n_shapes, f.rects.size(), e.n_rects, f.emitters.size(), e.n_emitters, f.n_tris, scene->d.n_tris);
    for (size_t i = 0; i < f.shapes.size(); ++i)
        if (f.shapes[i].rect < 0 && (f.shapes[i].material != e.shapes_host[i].material || f.shapes[i].emitter != e.shapes_host[i].emitter))
            return fail(BF_ERR_UNSUPPORTED, "bf_scene_update_endpoints: mesh shape %zu changed its material / emitter index (the "
                                            "triangle records carry them); create a new scene", i);
    if (scene->d.n_tris && f.origin_scale > scene->mesh.origin_scale_built)
        return fail(BF_ERR_UNSUPPORTED, "bf_scene_update_endpoints: an endpoint moved to |coordinate| %g, outside the bound %g the "
                                        "BVH boxes were padded for; create a new scene", (double) f.origin_scale,
                    (double) scene->mesh.origin_scale_built);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    // The paths of an open rolling sequence belong to the endpoints as they are.  Round 3 finished them first (a flush: one
    // tail per frame of a sweep whose radar turns — the loop the reference ships).  Now the update JOINS the sequence: the
    // new tables go into the next block of the handle's pool, the renders issued so far keep reading theirs through the
    // descriptor ring (kMulti kernels).  Phased arrays (their element tables are replaced in place), wide reconstruction
    // filters (no kMulti | kWide kernels), another stream or a full pool fall back to the flush.
    bool phased = f.sensor.type == BF_RECEIVER_PHASED || e.sensor_array_dev != nullptr;
    for (const auto &em : f.emitters) phased = phased || em.type == BF_TRANSMITTER_PHASED;
    for (float *p : e.array_dev) phased = phased || p != nullptr;
    const bool join = scene->run.roll.open && scene->run.roll.stream == stream && !phased && e.sensor_host.filt_n == 0u && f.sensor.filt_n == 0u &&
                      e.next + 1u < bfd::kRollRing && scene->tun.roll_join && any_resample_of(f.emitters) == e.any_resample;
    if ((st = order_after_last(scene, stream)) != BF_OK) return st;
    if (!join && (st = close_sequence(scene, stream)) != BF_OK) return st;
    if ((st = bind_arrays(scene, f, stream, false)) != BF_OK) return st;
    // The tables are packed into one pinned staging slot owned by the scene (the flattened records above are stack locals and
    // `desc` is the caller's) and copied in stream order — no host-blocking copy, nothing read after this call returns — to the
    // home block, or — joining an open sequence — to the next block of the pool.
    char *dst = e.home;
    if (join && (st = e.claim(&dst)) != BF_OK) return st;
    bf_scene::Stage *stg = nullptr;
    if ((st = stage_acquire(scene, e.lay.total, &stg)) != BF_OK) return st;
    e.pack(f, (char *) stg->host);
    HIP_TRY(hipMemcpyAsync(dst, stg->host, e.lay.total, hipMemcpyHostToDevice, stream));
    if ((st = stage_release_after(stg, stream)) != BF_OK) return st;
    e.point_at(dst);
    if (join) {
        e.joined();
        scene->run.roll.multi = true;
    }
    e.apply(f, scene->tun.tab_cache);      // (lean_profile reads the profile at the next render)
    return mark_last(scene, stream);
}

// The handle's class table (BF_FLAG_CLASSES): shape_class[n_shapes] in a device array of the handle's own, allocated at the first call and
// rewritten in stream order through the staging ring; the array's address, the number of classes and the miss class travel in the
// kernel arguments (bf_device.h: DScene::class_lo / class_hi / class_info), which every later render of the handle reads.
bf_status bf_scene_set_classes(bf_scene *scene, uint32_t n_classes, const uint32_t *shape_class, uint32_t miss_class, void *stream_) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_set_classes: null scene");
    const uint32_t n_shapes = scene->info.n_shapes;
    if (n_classes > BF_MAX_CLASSES) return fail(BF_ERR_INVALID, "bf_scene_set_classes: n_classes %u exceeds BF_MAX_CLASSES (%u)", n_classes, (unsigned) BF_MAX_CLASSES);
    if (n_classes) {
        if (n_shapes && !shape_class) return fail(BF_ERR_INVALID, "bf_scene_set_classes: shape_class is null");
        if (miss_class >= n_classes) return fail(BF_ERR_INVALID, "bf_scene_set_classes: miss_class %u is not below n_classes %u", miss_class, n_classes);
        for (uint32_t i = 0; i < n_shapes; ++i)
            if (shape_class[i] >= n_classes)
                return fail(BF_ERR_INVALID, "bf_scene_set_classes: shape_class[%u] = %u is not below n_classes %u", i, shape_class[i], n_classes);
    }
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    return install_classes(scene, shape_class, n_classes ? sizeof(uint32_t) * n_shapes : 0u, n_classes ? (n_classes | (miss_class << 16)) : 0u, stream);
}

// The table's arrival form: the twelve words of bfa::Table (bf_arrival.h) in the same device array, the form in bit 31 of class_info;
// miss_class is the class outside the window.  The scales are computed here, once.
bf_status bf_scene_set_arrival_classes(bf_scene *scene, const bf_arrival_bins *bins, void *stream_) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: null scene");
    if (!bins) return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: null bins");
    if (bins->n_u == 0 || bins->n_v == 0) return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: n_u = %u, n_v = %u: both must be at least 1", bins->n_u, bins->n_v);
    if ((uint64_t) bins->n_u * bins->n_v + 1u > BF_MAX_CLASSES)
        return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: %u x %u bins and the class outside the window exceed BF_MAX_CLASSES (%u)", bins->n_u,
                    bins->n_v, (unsigned) BF_MAX_CLASSES);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(bins->axis_u[i]) || !std::isfinite(bins->axis_v[i]))
            return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: an axis component is not finite");
    if (!std::isfinite(bins->u0) || !std::isfinite(bins->u1) || !std::isfinite(bins->v0) || !std::isfinite(bins->v1))
        return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: a window edge is not finite");
    if (!(bins->u1 > bins->u0) || !(bins->v1 > bins->v0))
        return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: the window [%g, %g) x [%g, %g) is empty", (double) bins->u0, (double) bins->u1,
                    (double) bins->v0, (double) bins->v1);
    bfa::Table t;
    std::memcpy(t.axis_u, bins->axis_u, sizeof(t.axis_u));
    std::memcpy(t.axis_v, bins->axis_v, sizeof(t.axis_v));
    t.u0 = bins->u0;
    t.v0 = bins->v0;
    t.su = bfa::scale(bins->n_u, bins->u0, bins->u1);
    t.sv = bfa::scale(bins->n_v, bins->v0, bins->v1);
    t.n_u = bins->n_u;
    t.n_v = bins->n_v;
    if (!std::isfinite(t.su) || !std::isfinite(t.sv))
        return fail(BF_ERR_INVALID, "bf_scene_set_arrival_classes: the scale n / (upper - lower) of a window axis is not finite (%g, %g)", (double) t.su,
                    (double) t.sv);
    const uint32_t outside = bins->n_u * bins->n_v;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    return install_classes(scene, &t, sizeof(t), (outside + 1u) | (outside << 16) | bfd::kClassArrival, stream);
}

// The table's range-rate form: bfr::Header and one bfr::Row per shape (bf_range_rate.h) in the same device array, the form in bit 30 of
// class_info; miss_class is n_bins + 1, the class of a path whose first ray leaves the scene, and n_bins the class of a rate outside the
// window.  The scale is computed here, once.
bf_status bf_scene_set_range_rate_classes(bf_scene *scene, const bf_range_rate_bins *bins, const bf_twist *twists, void *stream_) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: null scene");
    if (!bins) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: null bins");
    const uint32_t n_shapes = scene->info.n_shapes;
    if (n_shapes && !twists) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: twists is null");
    if (bins->n_bins == 0) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: n_bins = 0: must be at least 1");
    if ((uint64_t) bins->n_bins + 2u > BF_MAX_CLASSES)
        return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: %u bins, the class outside the window and the miss class exceed BF_MAX_CLASSES (%u)",
                    bins->n_bins, (unsigned) BF_MAX_CLASSES);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(bins->sensor_lin[i])) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: a sensor_lin component is not finite");
    if (!std::isfinite(bins->r0) || !std::isfinite(bins->r1)) return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: a window edge is not finite");
    if (!(bins->r1 > bins->r0))
        return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: the window [%g, %g) is empty", (double) bins->r0, (double) bins->r1);
    for (uint32_t k = 0; k < n_shapes; ++k)
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(twists[k].lin[i]) || !std::isfinite(twists[k].ang[i]) || !std::isfinite(twists[k].pivot[i]))
                return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: twists[%u] has a component that is not finite", k);
    std::vector<uint32_t> words((size_t) bfr::table_words(n_shapes), 0u);
    bfr::Header h = {};
    std::memcpy(h.sensor_lin, bins->sensor_lin, sizeof(h.sensor_lin));
    h.r0 = bins->r0;
    h.sr = bfa::scale(bins->n_bins, bins->r0, bins->r1);
    h.n_bins = bins->n_bins;
    if (!std::isfinite(h.sr))
        return fail(BF_ERR_INVALID, "bf_scene_set_range_rate_classes: the scale n_bins / (r1 - r0) of the window is not finite (%g)", (double) h.sr);
    std::memcpy(words.data(), &h, sizeof(h));
    for (uint32_t k = 0; k < n_shapes; ++k) {
        bfr::Row r = {};
        std::memcpy(r.lin, twists[k].lin, sizeof(r.lin));
        std::memcpy(r.ang, twists[k].ang, sizeof(r.ang));
        std::memcpy(r.pivot, twists[k].pivot, sizeof(r.pivot));
        std::memcpy(words.data() + bfr::kHeaderWords + (size_t) bfr::kRowWords * k, &r, sizeof(r));
    }
    const uint32_t outside = bins->n_bins;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    velocity_patch(scene, words, scene->mesh.vel);
    const bf_status st = install_classes(scene, words.data(), sizeof(uint32_t) * words.size(), (outside + 2u) | ((outside + 1u) << 16) | bfd::kClassRangeRate, stream);
    if (st == BF_OK) scene->ends.rr_words = std::move(words);
    return st;
}

}  // extern "C"
