// rm_addon.cc -- N-API binding of the C ABI (include/rm_raymarch.h) for a Node / Electron /
// worker_threads host of the reference's TypeScript.  It is the binding INTEGRATION.md
// describes: the worker keeps `Job` / `Result` (src/workers/raymarchWorker.ts:10-31) and
// replaces the body of onmessage (raymarchWorker.ts:33-92) with renderTile(job, buffers).
//
// One rm_ctx per addon INSTANCE, i.e. per napi_env: node loads the addon once per worker_threads
// worker (the .so itself is mapped once per process), so each worker of the reference's pool
// (main.ts:318-321) owns its own context.  The ABI is not thread-safe per ctx; nothing here is
// process-global.  The ctx lives in the env's instance data and is destroyed when the env goes.
// Nothing here throws: every call returns the rm_status code (0 ok, -2 = RM_E_UNSUPPORTED ->
// the caller keeps its CPU path for that job), lastError() has the text.
#define NAPI_VERSION 6  // napi_set_instance_data (node >= 12.17)
#include <node_api.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../include/rm_raymarch.h"

namespace {

struct Addon {
    rm_ctx *ctx = nullptr;
};

void addon_finalize(napi_env, void *data, void *) {
    Addon *a = static_cast<Addon *>(data);
    if (a->ctx) rm_destroy(a->ctx);
    delete a;
}

Addon *addon_of(napi_env env) {
    void *data = nullptr;
    if (napi_get_instance_data(env, &data) != napi_ok) return nullptr;
    return static_cast<Addon *>(data);
}

double num_prop(napi_env env, napi_value obj, const char *name, double dflt) {
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return dflt;
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return dflt;
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_number) return dflt;
    double d = dflt;
    napi_get_value_double(env, v, &d);
    return d;
}

std::string str_prop(napi_env env, napi_value obj, const char *name) {
    napi_value v;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return "";
    if (napi_get_named_property(env, obj, name, &v) != napi_ok) return "";
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok || t != napi_string) return "";
    char buf[64];
    size_t n = 0;
    napi_get_value_string_utf8(env, v, buf, sizeof buf, &n);
    return std::string(buf, n);
}

napi_value obj_prop(napi_env env, napi_value obj, const char *name) {
    napi_value v = nullptr;
    bool has = false;
    if (napi_has_named_property(env, obj, name, &has) == napi_ok && has) napi_get_named_property(env, obj, name, &v);
    return v;
}

// Job (raymarchWorker.ts:10-22) -> rm_job
rm_job job_from_js(napi_env env, napi_value j) {
    rm_job job;
    std::memset(&job, 0, sizeof job);
    job.width = static_cast<int32_t>(num_prop(env, j, "width", 0));
    job.height = static_cast<int32_t>(num_prop(env, j, "height", 0));
    job.time = num_prop(env, j, "time", 0);
    job.y_start = static_cast<int32_t>(num_prop(env, j, "yStart", 0));
    job.y_end = static_cast<int32_t>(num_prop(env, j, "yEnd", job.height));
    napi_value cam = obj_prop(env, j, "camera");
    if (cam) {
        job.camera_pitch = num_prop(env, cam, "pitch", 0);
        job.camera_yaw = num_prop(env, cam, "yaw", 0);
    }
    job.algorithm = rm_algorithm_from_string(str_prop(env, j, "algorithm").c_str());
    job.scene_preset_index = static_cast<int32_t>(num_prop(env, j, "scenePresetIndex", 0));
    job.acceleration_structure = rm_accel_from_string(str_prop(env, j, "accelerationStructure").c_str());
    job.overshoot_factor = num_prop(env, j, "overshootFactor", NAN);  // undefined -> constructor default
    job.step_size = num_prop(env, j, "stepSize", NAN);
    return job;
}

// typed array -> data pointer + byte length (nullptr when it is not a typed array)
void *typed(napi_env env, napi_value v, size_t *bytes) {
    bool is = false;
    *bytes = 0;
    if (!v || napi_is_typedarray(env, v, &is) != napi_ok || !is) return nullptr;
    napi_typedarray_type t;
    size_t len = 0, off = 0;
    void *data = nullptr;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off) != napi_ok) return nullptr;
    const size_t esz = (t == napi_uint16_array || t == napi_int16_array) ? 2
                       : (t == napi_uint8_array || t == napi_uint8_clamped_array || t == napi_int8_array) ? 1
                       : (t == napi_float64_array || t == napi_bigint64_array || t == napi_biguint64_array) ? 8 : 4;
    *bytes = len * esz;
    return data;
}

napi_value make_int(napi_env env, int v) {
    napi_value out;
    napi_create_int32(env, v, &out);
    return out;
}

// create(device) -> status
napi_value Create(napi_env env, napi_callback_info info) {
    size_t argc = 1;
    napi_value a[1];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    int32_t dev = 0;
    if (argc >= 1) napi_get_value_int32(env, a[0], &dev);
    Addon *ad = addon_of(env);
    if (!ad) return make_int(env, RM_E_INVALID);
    if (ad->ctx) {  // this env's own context only: another worker's context is never touched
        rm_destroy(ad->ctx);
        ad->ctx = nullptr;
    }
    return make_int(env, rm_create(dev, &ad->ctx));
}

// renderTile(job, depth: Uint8ClampedArray, normal: Uint8ClampedArray, sdfEval: Uint16Array, iters: Uint16Array)
napi_value RenderTile(napi_env env, napi_callback_info info) {
    size_t argc = 5;
    napi_value a[5];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx || argc < 5) return make_int(env, RM_E_INVALID);
    const rm_job job = job_from_js(env, a[0]);
    const size_t rows = job.y_end > job.y_start ? static_cast<size_t>(job.y_end - job.y_start) : 0;
    const size_t npx = rows * static_cast<size_t>(job.width > 0 ? job.width : 0);
    size_t b0, b1, b2, b3;
    uint8_t *depth = static_cast<uint8_t *>(typed(env, a[1], &b0));
    uint8_t *normal = static_cast<uint8_t *>(typed(env, a[2], &b1));
    uint16_t *sdf = static_cast<uint16_t *>(typed(env, a[3], &b2));
    uint16_t *iters = static_cast<uint16_t *>(typed(env, a[4], &b3));
    if (b0 < npx || b1 < 3 * npx || b2 < 2 * npx || b3 < 2 * npx) return make_int(env, RM_E_INVALID);
    return make_int(env, rm_render_tile(g_ctx, &job, depth, normal, sdf, iters));
}

// shade(modelName, width, height, depth, normal, sdfEval, iters, rgba)   (shadingModel.ts:8-17)
napi_value Shade(napi_env env, napi_callback_info info) {
    size_t argc = 8;
    napi_value a[8];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx || argc < 8) return make_int(env, RM_E_INVALID);
    char name[64];
    size_t n = 0;
    napi_get_value_string_utf8(env, a[0], name, sizeof name, &n);
    int32_t w = 0, h = 0;
    napi_get_value_int32(env, a[1], &w);
    napi_get_value_int32(env, a[2], &h);
    const size_t npx = static_cast<size_t>(w > 0 ? w : 0) * static_cast<size_t>(h > 0 ? h : 0);
    size_t b[5];
    void *p[5];
    for (int i = 0; i < 5; ++i) p[i] = typed(env, a[3 + i], &b[i]);
    if (b[0] < npx || b[1] < 3 * npx || b[2] < 2 * npx || b[3] < 2 * npx || b[4] < 4 * npx) return make_int(env, RM_E_INVALID);
    return make_int(env, rm_shade(g_ctx, rm_shader_from_string(name), w, h, static_cast<uint8_t *>(p[0]),
                                  static_cast<uint8_t *>(p[1]), static_cast<uint16_t *>(p[2]),
                                  static_cast<uint16_t *>(p[3]), static_cast<uint8_t *>(p[4])));
}

// diagnostics(sdfEval, iters) -> {totalSDFCalls, maxSDFCalls, minSDFCalls, totalIterations, totalPixels} | status
napi_value Diagnostics(napi_env env, napi_callback_info info) {
    size_t argc = 2;
    napi_value a[2];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx || argc < 2) return make_int(env, RM_E_INVALID);
    size_t b0, b1;
    uint16_t *sdf = static_cast<uint16_t *>(typed(env, a[0], &b0));
    uint16_t *iters = static_cast<uint16_t *>(typed(env, a[1], &b1));
    if (b0 != b1) return make_int(env, RM_E_INVALID);
    rm_diagnostics d;
    const int rc = rm_reduce_counters(g_ctx, sdf, iters, static_cast<int64_t>(b0 / 2), &d);
    if (rc) return make_int(env, rc);
    napi_value out, v;
    napi_create_object(env, &out);
    napi_create_double(env, static_cast<double>(d.total_sdf_calls), &v);
    napi_set_named_property(env, out, "totalSDFCalls", v);
    napi_create_double(env, static_cast<double>(d.max_sdf_calls), &v);
    napi_set_named_property(env, out, "maxSDFCalls", v);
    napi_create_double(env, static_cast<double>(d.min_sdf_calls), &v);
    napi_set_named_property(env, out, "minSDFCalls", v);
    napi_create_double(env, static_cast<double>(d.total_iterations), &v);
    napi_set_named_property(env, out, "totalIterations", v);
    napi_create_double(env, static_cast<double>(d.total_pixels), &v);
    napi_set_named_property(env, out, "totalPixels", v);
    return out;
}

// compareFrames(a, b, width, rows, nFrames, map, gain, rgba, stats) -> status   (rm_compare_frames, host buffers)
// a, b: {depth, normal, sdfEval, iters}, each a typed array or absent on both sides; map: rm_compare_map; rgba:
// Uint8ClampedArray or null (map -1); stats: null or a typed array of 128 bytes per frame that receives the rm_compare_stats records
napi_value CompareFrames(napi_env env, napi_callback_info info) {
    size_t argc = 9;
    napi_value a[9];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx || argc < 9) return make_int(env, RM_E_INVALID);
    int32_t v[5] = {0, 0, 0, 0, 0};  // width, rows, nFrames, map, gain
    for (int i = 0; i < 5; ++i) napi_get_value_int32(env, a[2 + i], &v[i]);
    const size_t n = v[2] > 0 ? static_cast<size_t>(v[2]) : 0;
    const size_t total = static_cast<size_t>(v[0] > 0 ? v[0] : 0) * static_cast<size_t>(v[1] > 0 ? v[1] : 0) * n;
    static const char *const names[4] = {"depth", "normal", "sdfEval", "iters"};
    const size_t bpp[4] = {1, 3, 2, 2};
    rm_frame_set sets[2];
    for (int side = 0; side < 2; ++side) {
        napi_valuetype t;
        if (napi_typeof(env, a[side], &t) != napi_ok || t != napi_object) return make_int(env, RM_E_INVALID);
        const void *p[4];
        for (int k = 0; k < 4; ++k) {
            size_t bytes = 0;
            p[k] = typed(env, obj_prop(env, a[side], names[k]), &bytes);
            if (p[k] && bytes < bpp[k] * total) return make_int(env, RM_E_INVALID);
        }
        sets[side] = rm_frame_set{p[0], p[1], p[2], p[3]};
    }
    size_t rgba_bytes = 0, stats_bytes = 0;
    uint8_t *rgba = static_cast<uint8_t *>(typed(env, a[7], &rgba_bytes));
    void *stats = typed(env, a[8], &stats_bytes);
    if ((rgba && rgba_bytes < 4 * total) || (stats && stats_bytes < sizeof(rm_compare_stats) * n)) return make_int(env, RM_E_INVALID);
    return make_int(env, rm_compare_frames(g_ctx, v[0], v[1], v[2], &sets[0], &sets[1], v[3], v[4], rgba, static_cast<rm_compare_stats *>(stats)));
}

// editSpheres(presetIndex, accelerationStructure, ops, spheres) -> status   (rm_scene_edit_spheres)
// Makes the scene a job with (presetIndex, accelerationStructure) would render the active one (RM_SCENE_UPLOADED: the scene
// edited before) and applies the edits to it: ops an Int32Array of (op, index) pairs, spheres a Float64Array of (x, y, z,
// radius) per edit (ignored by REMOVE).  Afterwards jobs select the edited scene with scenePresetIndex = RM_SCENE_UPLOADED.
napi_value EditSpheres(napi_env env, napi_callback_info info) {
    size_t argc = 4;
    napi_value a[4];
    napi_get_cb_info(env, info, &argc, a, nullptr, nullptr);
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx || argc < 4) return make_int(env, RM_E_INVALID);
    int32_t preset = 0;
    napi_get_value_int32(env, a[0], &preset);
    char accel[64];
    size_t len = 0;
    if (napi_get_value_string_utf8(env, a[1], accel, sizeof accel, &len) != napi_ok) accel[0] = 0;
    size_t ops_bytes = 0, sph_bytes = 0;
    const int32_t *ops = static_cast<const int32_t *>(typed(env, a[2], &ops_bytes));
    const double *sph = static_cast<const double *>(typed(env, a[3], &sph_bytes));
    const size_t n = ops_bytes / 8;
    if ((n && (!ops || !sph)) || ops_bytes % 8 || sph_bytes != 32 * n || n > 0x7FFFFFFF) return make_int(env, RM_E_INVALID);
    if (preset != RM_SCENE_UPLOADED) {
        const int rc = rm_scene_from_preset(g_ctx, preset, rm_accel_from_string(accel));
        if (rc) return make_int(env, rc);
    }
    std::string edits(n * sizeof(rm_sphere_edit), '\0');
    rm_sphere_edit *e = reinterpret_cast<rm_sphere_edit *>(&edits[0]);
    for (size_t i = 0; i < n; ++i) {
        e[i].op = ops[2 * i];
        e[i].index = ops[2 * i + 1];
        for (int k = 0; k < 3; ++k) e[i].center[k] = static_cast<float>(sph[4 * i + k]);
        e[i].reserved = 0;
        e[i].radius = sph[4 * i + 3];
    }
    return make_int(env, rm_scene_edit_spheres(g_ctx, n ? e : nullptr, static_cast<int32_t>(n)));
}

// sceneInfo() -> {nPrims, presetIndex, accel} | status   (rm_scene_get_info)
napi_value SceneInfo(napi_env env, napi_callback_info) {
    Addon *ad = addon_of(env);
    rm_ctx *g_ctx = ad ? ad->ctx : nullptr;
    if (!g_ctx) return make_int(env, RM_E_INVALID);
    rm_scene_info si;
    const int rc = rm_scene_get_info(g_ctx, &si);
    if (rc) return make_int(env, rc);
    napi_value out;
    napi_create_object(env, &out);
    napi_set_named_property(env, out, "nPrims", make_int(env, si.n_prims));
    napi_set_named_property(env, out, "presetIndex", make_int(env, si.preset_index));
    napi_set_named_property(env, out, "accel", make_int(env, si.accel));
    return out;
}

napi_value LastError(napi_env env, napi_callback_info) {
    napi_value out;
    Addon *ad = addon_of(env);
    const char *s = rm_last_error(ad ? ad->ctx : nullptr);
    napi_create_string_utf8(env, s, std::strlen(s), &out);
    return out;
}

napi_value Version(napi_env env, napi_callback_info) {
    napi_value out;
    const char *s = rm_version();
    napi_create_string_utf8(env, s, std::strlen(s), &out);
    return out;
}

napi_value Init(napi_env env, napi_value exports) {
    napi_set_instance_data(env, new Addon(), addon_finalize, nullptr);
    const napi_property_descriptor props[] = {
        {"create", nullptr, Create, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        {"renderTile", nullptr, RenderTile, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        {"shade", nullptr, Shade, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        {"diagnostics", nullptr, Diagnostics, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        {"lastError", nullptr, LastError, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        {"version", nullptr, Version, nullptr, nullptr, nullptr, napi_enumerable, nullptr},
        // (not enumerable: Object.keys of the addon stays the worker's surface of raymarchWorker.ts; hosts reach it through
        // FrameComparison of native/host/raymarcher.js)
        {"compareFrames", nullptr, CompareFrames, nullptr, nullptr, nullptr, napi_default, nullptr},
        // (likewise: Scene.editSpheres of native/host/raymarcher.js)
        {"editSpheres", nullptr, EditSpheres, nullptr, nullptr, nullptr, napi_default, nullptr},
        {"sceneInfo", nullptr, SceneInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
    };
    napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
    return exports;
}

}  // namespace

NAPI_MODULE(rm_addon, Init)
