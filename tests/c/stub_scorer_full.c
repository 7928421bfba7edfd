/* TEST INFRASTRUCTURE -- tests/c/stub_scorer.c completed to the whole of include/ssimu2_hip.h, so that the scoring
 * service (oavif_amd/csrc/oavif_scored.cpp) can be built and run on a machine without a GPU (tests/test_service_cpu.py)
 * and held against the same code linked directly.  It is NOT SSIMULACRA2.  Everything is a simple, exact function of the
 * bytes, restated in numpy by the test:
 *   samples are compared on the 16-bit scale, s16 = s * 65535 / (2^d - 1) (integer division; 8-bit: s * 257);
 *   8-bit calls:   score = 100 - 6 * SAD8 / (w*h*3)                      (stub_scorer.c's formula)
 *   16-bit calls:  score = 100 - 6 * SAD16 / (w*h*3) / 257, an 8-bit reference taken as s * 257, a 16-bit reference
 *                  seen by the 8-bit calls as s16 >> 8
 *   averages[k] = score + k (k < 108), scales = 1 + (w * h) % 6; batch item i likewise from its own score
 *   map[p] = |dR| + 0.5 |dG| + 0.25 |dB| of pixel p (8-bit differences), as float
 * ssimu2_version() is the value of STUB_SCORER_VERSION when that is set.
 * A 13 x 13 frame makes ssimu2_set_reference / ssimu2_score_rgb8 return SSIMU2_ERR_HIP (the service's fault path). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ssimu2_hip.h"

#define ssimu2_ctx_create stub_base_ctx_create
#define ssimu2_ctx_destroy stub_base_ctx_destroy
#define ssimu2_set_reference stub_base_set_reference
#define ssimu2_ctx_set_blur stub_base_set_blur
#define ssimu2_score_against_reference_strided stub_base_strided
#define ssimu2_score_against_reference stub_base_against
#define ssimu2_version stub_base_version
#include "stub_scorer.c"
#undef ssimu2_ctx_create
#undef ssimu2_ctx_destroy
#undef ssimu2_set_reference
#undef ssimu2_ctx_set_blur
#undef ssimu2_score_against_reference_strided
#undef ssimu2_score_against_reference
#undef ssimu2_version

typedef struct {
    ssimu2_ctx base; /* first: a full* is an ssimu2_ctx* */
    uint16_t* ref16; /* the reference on the 16-bit scale */
    int ref_hbd;
    double avg[108];
    int nscales;
    double* batch;
    uint32_t batch_n, batch_w, batch_h;
} full;

/* The service refuses a client whose library reports another version string: the test hands the product library's string
   to the stand-in through the environment. */
const char* ssimu2_version(void) {
    const char* v = getenv("STUB_SCORER_VERSION");
    return v && *v ? v : stub_base_version();
}

static int fail(ssimu2_ctx* c, int code, const char* what) {
    snprintf(c->err, sizeof c->err, "%s", what);
    return code;
}
static void note(full* f, double score, uint32_t w, uint32_t h) {
    for (int k = 0; k < 108; ++k) f->avg[k] = score + k;
    f->nscales = 1 + (int)(((uint64_t)w * h) % 6);
}
static void drop_ref(full* f) {
    free(f->base.ref);
    free(f->ref16);
    f->base.ref = NULL;
    f->ref16 = NULL;
}
static int check_args(ssimu2_ctx* c, const void* a, const void* b, uint32_t w, uint32_t h) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!a || !b) return fail(c, SSIMU2_ERR_INVALID_ARG, "null image pointer");
    if (w == 0 || h == 0) return fail(c, SSIMU2_ERR_INVALID_ARG, "zero image dimension");
    if ((uint64_t)w * h > (1ull << 31) / 3) return fail(c, SSIMU2_ERR_INVALID_ARG, "image larger than 2^31/3 pixels");
    return SSIMU2_OK;
}
static int check16(ssimu2_ctx* c, const void* px, uint32_t depth) {
    if (!px) return fail(c, SSIMU2_ERR_INVALID_ARG, "null image pointer");
    if ((uintptr_t)px & 1u) return fail(c, SSIMU2_ERR_INVALID_ARG, "16-bit image pointer not 2-byte aligned");
    if (depth < 8 || depth > 16) return fail(c, SSIMU2_ERR_UNSUPPORTED, "bit_depth must be 8..16");
    return SSIMU2_OK;
}
static uint32_t s16(uint32_t s, uint32_t depth) {
    const uint32_t maxv = (1u << depth) - 1u;
    return (s > maxv ? maxv : s) * 65535u / maxv;
}

int ssimu2_ctx_create(int device, void* hip_stream, ssimu2_ctx** out_ctx) {
    (void)device; (void)hip_stream;
    if (!out_ctx) return SSIMU2_ERR_INVALID_ARG;
    *out_ctx = (ssimu2_ctx*)calloc(1, sizeof(full));
    return *out_ctx ? SSIMU2_OK : SSIMU2_ERR_OOM;
}
void ssimu2_ctx_destroy(ssimu2_ctx* c) {
    full* f = (full*)c;
    if (!f) return;
    drop_ref(f);
    free(f->batch);
    free(f);
}
int ssimu2_ctx_set_blur(ssimu2_ctx* c, int mode) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (mode < 0 || mode > 2) return fail(c, SSIMU2_ERR_INVALID_ARG, "unknown blur mode");
    c->blur = mode;
    drop_ref((full*)c);
    return SSIMU2_OK;
}
int ssimu2_query_device(int device, ssimu2_device_info* out) {
    if (!out || out->struct_size != sizeof *out) return SSIMU2_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->struct_size = (uint32_t)sizeof *out;
    out->device = device;
    snprintf(out->arch, sizeof out->arch, "stub");
    snprintf(out->name, sizeof out->name, "stub scorer");
    snprintf(out->pci_bus_id, sizeof out->pci_bus_id, "0000:00:00.0");
    out->compute_units = 1;
    out->wavefront_size = 64;
    out->numa_node = -1;
    out->usable = 1;
    return SSIMU2_OK;
}
int ssimu2_ctx_device_info(const ssimu2_ctx* c, ssimu2_device_info* out) {
    return c ? ssimu2_query_device(0, out) : SSIMU2_ERR_INVALID_ARG;
}

static int store_ref16(full* f, const void* px, int wide, uint32_t w, uint32_t h, uint32_t depth) {
    const size_t n = (size_t)w * h * 3;
    drop_ref(f);
    f->base.ref = (uint8_t*)malloc(n);
    f->ref16 = (uint16_t*)malloc(n * 2);
    if (!f->base.ref || !f->ref16) { drop_ref(f); return fail(&f->base, SSIMU2_ERR_OOM, "malloc"); }
    for (size_t i = 0; i < n; ++i) {
        f->ref16[i] = (uint16_t)(wide ? s16(((const uint16_t*)px)[i], depth) : ((const uint8_t*)px)[i] * 257u);
        f->base.ref[i] = (uint8_t)(f->ref16[i] >> 8);
    }
    f->base.w = w; f->base.h = h; f->ref_hbd = wide;
    return SSIMU2_OK;
}
int ssimu2_set_reference(ssimu2_ctx* c, const uint8_t* ref, uint32_t w, uint32_t h) {
    int rc = check_args(c, ref, ref, w, h);
    if (rc) return rc;
    if (w == 13 && h == 13) return fail(c, SSIMU2_ERR_HIP, "stub: injected HIP error");
    return store_ref16((full*)c, ref, 0, w, h, 8);
}
int ssimu2_set_reference_rgb16(ssimu2_ctx* c, const uint16_t* ref, uint32_t w, uint32_t h, uint32_t depth) {
    int rc = check_args(c, ref, ref, w, h);
    if (rc || (rc = check16(c, ref, depth))) return rc;
    return store_ref16((full*)c, ref, 1, w, h, depth);
}
int ssimu2_score_against_reference_strided(ssimu2_ctx* c, const uint8_t* px, uint32_t row_bytes, uint32_t channels, double* out) {
    const int rc = stub_base_strided(c, px, row_bytes, channels, out);
    if (rc == SSIMU2_OK) note((full*)c, *out, c->w, c->h);
    return rc;
}
int ssimu2_score_against_reference(ssimu2_ctx* c, const uint8_t* dist, double* out) {
    return c ? ssimu2_score_against_reference_strided(c, dist, c->w * 3, 3, out) : SSIMU2_ERR_INVALID_ARG;
}
int ssimu2_score_rgb8(ssimu2_ctx* c, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                      double* out) {
    int rc = check_args(c, ref, dist, w, h);
    if (rc) return rc;
    if (channels != 3) return fail(c, SSIMU2_ERR_UNSUPPORTED, "channels must be 3");
    if (!out) return fail(c, SSIMU2_ERR_INVALID_ARG, "null out_score");
    if (w == 13 && h == 13) return fail(c, SSIMU2_ERR_HIP, "stub: injected HIP error");
    if ((rc = store_ref16((full*)c, ref, 0, w, h, 8))) return rc;
    rc = ssimu2_score_against_reference(c, dist, out);
    drop_ref((full*)c); /* a pair score leaves no reference */
    return rc;
}

/* one 16-bit frame against ref16 */
static int against16(full* f, const uint16_t* px, uint32_t row_bytes, uint32_t channels, uint32_t depth, double* out) {
    const uint32_t w = f->base.w, h = f->base.h;
    unsigned long long sad = 0;
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
            for (uint32_t k = 0; k < 3; ++k) {
                const uint16_t* row = (const uint16_t*)((const uint8_t*)px + (size_t)y * row_bytes);
                const int d = (int)s16(row[(size_t)x * channels + k], depth) - (int)f->ref16[((size_t)y * w + x) * 3 + k];
                sad += (unsigned)(d < 0 ? -d : d);
            }
    *out = 100.0 - 6.0 * (double)sad / ((double)w * h * 3) / 257.0;
    note(f, *out, w, h);
    return SSIMU2_OK;
}
static int check_against(ssimu2_ctx* c, int pointers) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!c->ref) return fail(c, SSIMU2_ERR_NO_REFERENCE, "no reference set");
    if (!pointers) return fail(c, SSIMU2_ERR_INVALID_ARG, "null pointer");
    return SSIMU2_OK;
}
int ssimu2_score_against_reference_strided16(ssimu2_ctx* c, const uint16_t* px, uint32_t row_bytes, uint32_t channels,
                                             uint32_t depth, double* out) {
    int rc = check_against(c, out != NULL);
    if (rc || (rc = check16(c, px, depth))) return rc;
    if (channels != 3 && channels != 4) return fail(c, SSIMU2_ERR_UNSUPPORTED, "channels must be 3 (RGB) or 4 (RGBA)");
    if ((row_bytes & 1u) || (uint64_t)row_bytes < (uint64_t)c->w * channels * 2)
        return fail(c, SSIMU2_ERR_INVALID_ARG, "row_bytes odd or smaller than one row of 16-bit pixels");
    return against16((full*)c, px, row_bytes, channels, depth, out);
}
int ssimu2_score_against_reference_rgb16(ssimu2_ctx* c, const uint16_t* dist, uint32_t depth, double* out) {
    int rc = check_against(c, out != NULL);
    if (rc || (rc = check16(c, dist, depth))) return rc;
    return against16((full*)c, dist, c->w * 6u, 3, depth, out);
}
int ssimu2_score_rgb16(ssimu2_ctx* c, const uint16_t* ref, const uint16_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                       uint32_t depth, double* out) {
    int rc = check_args(c, ref, dist, w, h);
    if (rc || (rc = check16(c, ref, depth)) || (rc = check16(c, dist, depth))) return rc;
    if (channels != 3) return fail(c, SSIMU2_ERR_UNSUPPORTED, "channels must be 3");
    if (!out) return fail(c, SSIMU2_ERR_INVALID_ARG, "null out_score");
    if ((rc = store_ref16((full*)c, ref, 1, w, h, depth))) return rc;
    rc = against16((full*)c, dist, w * 6u, 3, depth, out);
    drop_ref((full*)c);
    return rc;
}

static void map8(const uint8_t* ref, const uint8_t* dist, size_t pixels, float* out) {
    for (size_t p = 0; p < pixels; ++p)
        out[p] = (float)abs(dist[3 * p] - ref[3 * p]) + 0.5f * (float)abs(dist[3 * p + 1] - ref[3 * p + 1]) +
                 0.25f * (float)abs(dist[3 * p + 2] - ref[3 * p + 2]);
}
int ssimu2_error_map_rgb8(ssimu2_ctx* c, const uint8_t* ref, const uint8_t* dist, uint32_t w, uint32_t h, uint32_t channels,
                          float* out_map, double* out) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!out_map) return fail(c, SSIMU2_ERR_INVALID_ARG, "null out_map");
    const int rc = ssimu2_score_rgb8(c, ref, dist, w, h, channels, out);
    if (rc) return rc;
    map8(ref, dist, (size_t)w * h, out_map);
    return SSIMU2_OK;
}
int ssimu2_error_map_against_reference(ssimu2_ctx* c, const uint8_t* dist, float* out_map, double* out) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (!out_map) return fail(c, SSIMU2_ERR_INVALID_ARG, "null out_map");
    if (c->ref && ((full*)c)->ref_hbd)
        return fail(c, SSIMU2_ERR_UNSUPPORTED, "no error map against a reference set from 16-bit samples");
    if (!c->ref) return fail(c, SSIMU2_ERR_NO_REFERENCE, "no reference set");
    if (!dist || !out) return fail(c, SSIMU2_ERR_INVALID_ARG, "null pointer");
    const int rc = ssimu2_score_against_reference(c, dist, out);
    if (rc) return rc;
    map8(c->ref, dist, (size_t)c->w * c->h, out_map);
    return SSIMU2_OK;
}
int ssimu2_last_averages(ssimu2_ctx* c, double* out, int* out_num_scales) {
    if (!c || !out) return SSIMU2_ERR_INVALID_ARG;
    memcpy(out, ((full*)c)->avg, sizeof ((full*)c)->avg);
    if (out_num_scales) *out_num_scales = ((full*)c)->nscales;
    return SSIMU2_OK;
}
int ssimu2_linear_table(uint32_t depth, float* out) {
    if (!out) return SSIMU2_ERR_INVALID_ARG;
    if (depth < 8 || depth > 16) return SSIMU2_ERR_UNSUPPORTED;
    for (uint32_t i = 0; i < (1u << depth); ++i) out[i] = (float)i / (float)((1u << depth) - 1u);
    return SSIMU2_OK;
}

/* batches: each item scored by the 8-bit formula, with scratch of its own (a cached reference stays) */
static int batch_open(ssimu2_ctx* c, uint32_t n, int against) {
    if (!c) return SSIMU2_ERR_INVALID_ARG;
    if (n == 0) return SSIMU2_OK;
    if (c->blur != SSIMU2_BLUR_FIR) return fail(c, SSIMU2_ERR_UNSUPPORTED, "batch scoring runs in SSIMU2_BLUR_FIR only");
    if (against && !c->ref) return fail(c, SSIMU2_ERR_NO_REFERENCE, "no reference set");
    if (n > SSIMU2_MAX_BATCH) return fail(c, SSIMU2_ERR_INVALID_ARG, "batch larger than SSIMU2_MAX_BATCH items");
    return SSIMU2_OK;
}
static int batch_run(full* f, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w, uint32_t h,
                     double* out) {
    double* keep = (double*)realloc(f->batch, (size_t)n * sizeof(double));
    if (!keep) return fail(&f->base, SSIMU2_ERR_OOM, "malloc");
    f->batch = keep;
    const size_t bytes = (size_t)w * h * 3;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* ref = refs ? refs[i] : f->base.ref;
        unsigned long long sad = 0;
        for (size_t k = 0; k < bytes; ++k) sad += (unsigned)abs((int)dists[i][k] - (int)ref[k]);
        out[i] = keep[i] = 100.0 - 6.0 * (double)sad / ((double)w * h * 3);
    }
    f->batch_n = n; f->batch_w = w; f->batch_h = h;
    return SSIMU2_OK;
}
int ssimu2_score_batch_rgb8(ssimu2_ctx* c, const uint8_t* const* refs, const uint8_t* const* dists, uint32_t n, uint32_t w,
                            uint32_t h, double* out) {
    int rc = batch_open(c, n, 0);
    if (rc || n == 0) return rc;
    if ((rc = check_args(c, refs, dists, w, h))) return rc;
    if (!out) return fail(c, SSIMU2_ERR_INVALID_ARG, "null out_scores");
    for (uint32_t i = 0; i < n; ++i)
        if (!refs[i] || !dists[i]) return fail(c, SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    return batch_run((full*)c, refs, dists, n, w, h, out);
}
int ssimu2_score_batch_against_reference(ssimu2_ctx* c, const uint8_t* const* dists, uint32_t n, double* out) {
    int rc = batch_open(c, n, 1);
    if (rc || n == 0) return rc;
    if (!dists || !out) return fail(c, SSIMU2_ERR_INVALID_ARG, "null pointer");
    for (uint32_t i = 0; i < n; ++i)
        if (!dists[i]) return fail(c, SSIMU2_ERR_INVALID_ARG, "null image pointer in the batch");
    return batch_run((full*)c, NULL, dists, n, c->w, c->h, out);
}
int ssimu2_last_batch_averages(ssimu2_ctx* c, uint32_t item, double* out, int* out_num_scales) {
    full* f = (full*)c;
    if (!c || !out) return SSIMU2_ERR_INVALID_ARG;
    if (item >= f->batch_n) return fail(c, SSIMU2_ERR_INVALID_ARG, "ssimu2_last_batch_averages: no such item in the last batch");
    for (int k = 0; k < 108; ++k) out[k] = f->batch[item] + k;
    if (out_num_scales) *out_num_scales = 1 + (int)(((uint64_t)f->batch_w * f->batch_h) % 6);
    return SSIMU2_OK;
}

/* the device-pointer and enqueue forms: nothing a CPU stand-in can do */
int ssimu2_score_rgb8_device(ssimu2_ctx* c, const void* a, const void* b, uint32_t w, uint32_t h, double* o) {
    (void)a; (void)b; (void)w; (void)h; (void)o;
    return c ? fail(c, SSIMU2_ERR_UNSUPPORTED, "stub: no device") : SSIMU2_ERR_INVALID_ARG;
}
int ssimu2_enqueue_rgb8_device(ssimu2_ctx* c, const void* a, const void* b, uint32_t w, uint32_t h) {
    return ssimu2_score_rgb8_device(c, a, b, w, h, NULL);
}
int ssimu2_wait(ssimu2_ctx* c, double* o) { return ssimu2_score_rgb8_device(c, NULL, NULL, 0, 0, o); }
int ssimu2_set_reference_device(ssimu2_ctx* c, const void* a, uint32_t w, uint32_t h) {
    return ssimu2_score_rgb8_device(c, a, a, w, h, NULL);
}
int ssimu2_enqueue_against_reference_device(ssimu2_ctx* c, const void* a) { return ssimu2_score_rgb8_device(c, a, a, 0, 0, NULL); }
int ssimu2_score_batch_rgb8_device(ssimu2_ctx* c, const void* a, const void* b, size_t s, uint32_t n, uint32_t w, uint32_t h,
                                   double* o) {
    (void)s; (void)n;
    return ssimu2_score_rgb8_device(c, a, b, w, h, o);
}
int ssimu2_score_batch_against_reference_device(ssimu2_ctx* c, const void* a, size_t s, uint32_t n, double* o) {
    (void)s; (void)n;
    return ssimu2_score_rgb8_device(c, a, a, 0, 0, o);
}
