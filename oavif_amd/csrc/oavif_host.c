/*
 * oavif_host.c -- the drop-in, end to end, as a compiled host: what oavif's main.zig does
 * around the boundary (/root/reference/src/main.zig:37-117), in C over the two public headers.
 *
 *     oavif_host [options] <in.png|in.pam> <out.avif>
 *
 * The reference's host language is Zig and the image has no Zig toolchain, so the binding a
 * maintainer adds (oavif_amd/zig/fssimu2.zig) cannot be compiled here.
 * This file is the same host side in the language that CAN be compiled here, with nothing of
 * Python in the loop:
 *
 *   main.zig:73-91    load the image, build the scorer's RGB8 reference (Image.toRGB8)
 *   main.zig:93-100   -q: encode once
 *   main.zig:102-116  findTargetQuality -> oavif_tq_find_target_quality (include/oavif_tq.h), whose
 *                     pass (tq.zig:21-38) is the callback below: io.encodeAvifToBuffer and
 *                     decodeAvifCommon against libavif's C API, call for call (io.zig:452-482,
 *                     544-636), then the score of tq.zig:37 on the GPU through
 *                     ssimu2_score_against_reference_strided (libavif's RGB(A) rows as they are:
 *                     the copy loop of io.zig:654-663 never runs)
 *   io.zig:550-617    the source is rescaled to the encoder's depth (oavif_prescale_*) and converted to
 *                     YUV444 ONCE, not once per pass (SURVEY.md 8f rank 4 and one step further)
 *
 * libavif: the image has a libavif 1.4.1 shared library (inside Pillow's wheel) and no header.
 * The leading members of the four public structs used here are declared below from the public
 * API of libavif 1.x, the library is opened with dlopen (OAVIF_LIBAVIF names it), and the
 * documented defaults of avifEncoderCreate / avifDecoderCreate / avifImageCreate /
 * avifRGBImageSetDefaults are read back through these declarations before anything is encoded:
 * a library with another layout is refused.  PNG input goes through oavif_png_decode (the C ABI's
 * loader with io.loadPNG's output rules), PAM through the reader below (io.zig:309-406).
 *
 * stderr carries the reference's lines in the reference's formats (main.zig:78-84,95,98,102,106,116:
 * scripts/measure.py parses "N passes").  Exit code 0, or 1 with "error: <ZigErrorName>".
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <errno.h>
#include <math.h>
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "oavif_tq.h"
#include "ssimu2_hip.h"

#define VERSION "oavif_amd-0.1 (C host)"

/* ---- libavif 1.x: the members this host touches (public API; checked at run time) --------------------- */
typedef struct { uint8_t* data; size_t size; } avifRWData;
typedef struct {
    uint32_t width, height, depth;
    int yuvFormat, yuvRange, yuvChromaSamplePosition;
    uint8_t* yuvPlanes[3];
    uint32_t yuvRowBytes[3];
    int imageOwnsYUVPlanes;
    uint8_t* alphaPlane;
    uint32_t alphaRowBytes;
    int imageOwnsAlphaPlane, alphaPremultiplied;
    avifRWData icc;
    uint16_t colorPrimaries, transferCharacteristics, matrixCoefficients;
} avifImageHead; /* avifImage continues (clli, transforms, exif, xmp, ...): never touched */
typedef struct {
    uint32_t width, height, depth;
    int format, chromaUpsampling, chromaDownsampling, avoidLibYUV, ignoreAlpha, alphaPremultiplied, isFloat;
    int maxThreads;
    uint8_t* pixels;
    uint32_t rowBytes;
} avifRGBImage;
typedef struct {
    int codecChoice, maxThreads, speed, keyframeInterval;
    uint64_t timescale;
    int repetitionCount;
    uint32_t extraLayerCount;
    int quality, qualityAlpha, minQuantizer, maxQuantizer, minQuantizerAlpha, maxQuantizerAlpha;
    int tileRowsLog2, tileColsLog2, autoTiling;
    int scalingMode[4];
} avifEncoderHead; /* avifEncoder continues (ioStats, diag, data, ...) */
typedef struct {
    int codecChoice, maxThreads, requestedSource, allowProgressive, allowIncremental, ignoreExif, ignoreXMP;
    uint32_t imageSizeLimit, imageDimensionLimit, imageCountLimit, strictFlags;
    avifImageHead* image;
} avifDecoderHead; /* avifDecoder continues */
_Static_assert(offsetof(avifImageHead, alphaPlane) == 64 && offsetof(avifImageHead, icc) == 88 &&
               offsetof(avifImageHead, colorPrimaries) == 104, "avifImage head");
_Static_assert(offsetof(avifRGBImage, pixels) == 48 && offsetof(avifRGBImage, rowBytes) == 56, "avifRGBImage");
_Static_assert(offsetof(avifEncoderHead, quality) == 32 && offsetof(avifEncoderHead, autoTiling) == 64, "avifEncoder head");
_Static_assert(offsetof(avifDecoderHead, image) == 48, "avifDecoder head");
enum { AVIF_OK = 0, AVIF_YUV444 = 1, AVIF_RGB = 0, AVIF_RGBA = 1, AVIF_ADD_IMAGE_FLAG_SINGLE = 2 };

static struct {
    const char* (*Version)(void);
    const char* (*ResultToString)(int);
    avifImageHead* (*ImageCreate)(uint32_t, uint32_t, uint32_t, int);
    void (*ImageDestroy)(avifImageHead*);
    int (*ImageSetProfileICC)(avifImageHead*, const uint8_t*, size_t);
    void (*RGBImageSetDefaults)(avifRGBImage*, const avifImageHead*);
    int (*RGBImageAllocatePixels)(avifRGBImage*);
    void (*RGBImageFreePixels)(avifRGBImage*);
    int (*ImageRGBToYUV)(avifImageHead*, const avifRGBImage*);
    int (*ImageYUVToRGB)(const avifImageHead*, avifRGBImage*);
    avifEncoderHead* (*EncoderCreate)(void);
    void (*EncoderDestroy)(avifEncoderHead*);
    int (*EncoderSetCodecSpecificOption)(avifEncoderHead*, const char*, const char*);
    int (*EncoderAddImage)(avifEncoderHead*, const avifImageHead*, uint64_t, uint32_t);
    int (*EncoderFinish)(avifEncoderHead*, avifRWData*);
    void (*RWDataFree)(avifRWData*);
    avifDecoderHead* (*DecoderCreate)(void);
    void (*DecoderDestroy)(avifDecoderHead*);
    int (*DecoderSetIOMemory)(avifDecoderHead*, const uint8_t*, size_t);
    int (*DecoderParse)(avifDecoderHead*);
    int (*DecoderNextImage)(avifDecoderHead*);
} av;

static const char* g_err = NULL; /* the reference's Zig error name of the failure (the first one: probes may run on threads) */
static char g_detail[320];
static pthread_mutex_t g_lock = PTHREAD_MUTEX_INITIALIZER;
static int fail(const char* name, const char* detail) {
    pthread_mutex_lock(&g_lock);
    if (!g_err) {
        g_err = name;
        snprintf(g_detail, sizeof g_detail, "%s", detail ? detail : "");
    }
    pthread_mutex_unlock(&g_lock);
    return -1;
}
static void forget_failure(void) { /* after a failure that was a question, not an error (supports_10bit) */
    g_err = NULL;
    g_detail[0] = 0;
}

/* ---- the environment, read once (run(); print_version for the library's name) ------------------------- */
typedef struct {
    const char* libavif; /* OAVIF_LIBAVIF: the library to open; NULL or "" = libavif.so */
    int pinned;          /* OAVIF_HOST_PINNED=0 switches the page-locked frame buffers off */
    int times;           /* OAVIF_HOST_TIMES: the phase timeline and the times: / speculative: lines */
    int blur;            /* OAVIF_SSIMU2_BLUR: the blur of the search path, the published recursion unless it says
                            otherwise (as the Zig shim's `blur` and the Python mirror: INTEGRATION.md section 2e) */
    int fanout;          /* OAVIF_PROBE_FANOUT, at most OAVIF_TQ_MAX_FANOUT; above 1 the probes of a search are fanned.
                            Not a CLI flag: the option surface stays the reference's (parse_args.zig:76-122) */
    int device;          /* LOCAL_RANK */
} Env;
static void env_read(Env* v) {
    const char *pinned = getenv("OAVIF_HOST_PINNED"), *bm = getenv("OAVIF_SSIMU2_BLUR");
    const char *fan = getenv("OAVIF_PROBE_FANOUT"), *rank = getenv("LOCAL_RANK");
    v->libavif = getenv("OAVIF_LIBAVIF");
    v->pinned = !(pinned && !strcmp(pinned, "0"));
    v->times = getenv("OAVIF_HOST_TIMES") != NULL;
    v->blur = SSIMU2_BLUR_RECURSIVE;
    if (bm && !strcmp(bm, "fir")) v->blur = SSIMU2_BLUR_FIR;
    else if (bm && (!strcmp(bm, "recursive_fma") || !strcmp(bm, "iir_fma"))) v->blur = SSIMU2_BLUR_RECURSIVE_FMA;
    v->fanout = fan ? atoi(fan) : 1;
    if (v->fanout > OAVIF_TQ_MAX_FANOUT) v->fanout = OAVIF_TQ_MAX_FANOUT;
    v->device = rank ? atoi(rank) : 0;
}

static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

static int load_libavif(const char* path) {
    void* h = dlopen(path && *path ? path : "libavif.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("libavif.so.16", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail("LibavifUnavailable", dlerror());
#define SYM(field, name)                                                    \
    do {                                                                    \
        *(void**)(&av.field) = dlsym(h, name);                              \
        if (!av.field) return fail("LibavifUnavailable", "missing " name);  \
    } while (0)
    SYM(Version, "avifVersion"); SYM(ResultToString, "avifResultToString");
    SYM(ImageCreate, "avifImageCreate"); SYM(ImageDestroy, "avifImageDestroy");
    SYM(ImageSetProfileICC, "avifImageSetProfileICC"); SYM(RGBImageSetDefaults, "avifRGBImageSetDefaults");
    SYM(RGBImageAllocatePixels, "avifRGBImageAllocatePixels"); SYM(RGBImageFreePixels, "avifRGBImageFreePixels");
    SYM(ImageRGBToYUV, "avifImageRGBToYUV"); SYM(ImageYUVToRGB, "avifImageYUVToRGB");
    SYM(EncoderCreate, "avifEncoderCreate"); SYM(EncoderDestroy, "avifEncoderDestroy");
    SYM(EncoderSetCodecSpecificOption, "avifEncoderSetCodecSpecificOption");
    SYM(EncoderAddImage, "avifEncoderAddImage"); SYM(EncoderFinish, "avifEncoderFinish");
    SYM(RWDataFree, "avifRWDataFree"); SYM(DecoderCreate, "avifDecoderCreate");
    SYM(DecoderDestroy, "avifDecoderDestroy"); SYM(DecoderSetIOMemory, "avifDecoderSetIOMemory");
    SYM(DecoderParse, "avifDecoderParse"); SYM(DecoderNextImage, "avifDecoderNextImage");
#undef SYM
    /* layout guard: the documented defaults, read back through the declarations above */
    if (strncmp(av.Version(), "1.", 2) != 0) return fail("LibavifUnavailable", "not libavif 1.x");
    avifEncoderHead* e = av.EncoderCreate();
    if (!e) return fail("OutOfMemory", NULL);
    const int enc_ok = e->codecChoice == 0 && e->maxThreads == 1 && e->speed == -1 && e->keyframeInterval == 0 &&
                       e->timescale == 1 && e->repetitionCount == -1 && e->extraLayerCount == 0 &&
                       e->minQuantizer == 0 && e->maxQuantizer == 63 && e->minQuantizerAlpha == 0 &&
                       e->maxQuantizerAlpha == 63 && e->tileRowsLog2 == 0 && e->tileColsLog2 == 0 &&
                       e->autoTiling == 0 && e->scalingMode[0] == 1 && e->scalingMode[1] == 1 &&
                       e->scalingMode[2] == 1 && e->scalingMode[3] == 1;
    av.EncoderDestroy(e);
    avifDecoderHead* d = av.DecoderCreate();
    if (!d) return fail("OutOfMemory", NULL);
    const int dec_ok = d->maxThreads == 1 && d->imageSizeLimit == 16384u * 16384u && d->imageDimensionLimit == 32768 &&
                       d->imageCountLimit == 12 * 3600 * 60 && d->image == NULL;
    av.DecoderDestroy(d);
    avifImageHead* im = av.ImageCreate(24, 16, 10, AVIF_YUV444);
    if (!im) return fail("OutOfMemory", NULL);
    avifRGBImage rgb;
    memset(&rgb, 0xaa, sizeof rgb);
    av.RGBImageSetDefaults(&rgb, im);
    const int img_ok = im->width == 24 && im->height == 16 && im->depth == 10 && im->yuvFormat == AVIF_YUV444 &&
                       im->yuvRange == 1 && im->alphaPlane == NULL && im->icc.data == NULL && im->icc.size == 0 &&
                       im->colorPrimaries == 2 && im->transferCharacteristics == 2 && im->matrixCoefficients == 2;
    const int rgb_ok = rgb.width == 24 && rgb.height == 16 && rgb.depth == 10 && rgb.format == AVIF_RGBA &&
                       rgb.maxThreads == 1 && rgb.pixels == NULL && rgb.rowBytes == 0;
    av.ImageDestroy(im);
    if (!(enc_ok && dec_ok && img_ok && rgb_ok))
        return fail("LibavifUnavailable", "struct layout of the loaded libavif differs from the 1.x one declared here");
    return 0;
}

/* ---- options (parse_args.zig:48-63 defaults, :76-122 flags and ranges) ----------------------------------- */
typedef struct {
    int quality_alpha, speed, max_threads, tile_rows_log2, tile_cols_log2, auto_tiling;
    double score_tgt;
    int tenbit;
    const char* tune;
    double tolerance;
    int max_pass, quality /* -1 = search */, color_primaries, transfer_characteristics, matrix_coefficients;
} Options;
#define OPTIONS_DEFAULT {0, 9, 1, 0, 0, 1, 80.0, 1, "iq", 2.0, 6, -1, 2, 2, 2} /* parse_args.zig:48-63 */

static const char* arg_value(int* i, int argc, char** argv, const char* name) { /* the next argument, consumed */
    if (*i >= argc || argv[*i][0] == '-') { /* parse_args.zig:126: a value starting with '-' counts as missing */
        fprintf(stderr, "Error: Missing %s value\n", name);
        fail("MissingOptionValue", NULL);
        return NULL;
    }
    return argv[(*i)++];
}
static int int_arg(int* i, int argc, char** argv, long lo, long hi, const char* name, int* out) {
    const char* a = arg_value(i, argc, argv, name);
    if (!a) return -1;
    char* end;
    errno = 0;
    const long v = strtol(a, &end, 10);
    if (*end || errno) return fail("InvalidCharacter", NULL);
    if (v < lo || v > hi) {
        fprintf(stderr, "Error: %s must be between %ld and %ld\n", name, lo, hi);
        return fail("InvalidOptionValue", NULL);
    }
    *out = (int)v;
    return 0;
}
static int float_arg(int* i, int argc, char** argv, double lo, double hi, const char* name, double* out) {
    const char* a = arg_value(i, argc, argv, name);
    if (!a) return -1;
    char* end;
    const double v = strtod(a, &end);
    if (*end || end == a) return fail("InvalidCharacter", NULL);
    if (v < lo || v > hi) {
        fprintf(stderr, "Error: %s must be between %g and %g\n", name, lo, hi);
        return fail("InvalidOptionValue", NULL);
    }
    *out = v;
    return 0;
}
static int bool_arg(int* i, int argc, char** argv, const char* name, int* out) {
    const char* a = arg_value(i, argc, argv, name);
    if (!a) return -1;
    if (strcmp(a, "0") != 0 && strcmp(a, "1") != 0) {
        fprintf(stderr, "Error: %s must be 0 or 1\n", name);
        return fail("InvalidOptionValue", NULL);
    }
    *out = a[0] == '1';
    return 0;
}

static int parse_args(Options* o, int argc, char** argv, const char** in, const char** out) {
    for (int i = 1; i < argc;) {
        const char* a = argv[i++];
#define IS(s) (strcmp(a, s) == 0)
        int rc = 0;
        if (IS("-s") || IS("--speed")) rc = int_arg(&i, argc, argv, 0, 10, "--speed", &o->speed);
        else if (IS("-t") || IS("--score-tgt")) rc = float_arg(&i, argc, argv, 30, 100, "--score-tgt", &o->score_tgt);
        else if (IS("--quality-alpha")) rc = int_arg(&i, argc, argv, 0, 99, "--quality-alpha", &o->quality_alpha);
        else if (IS("--max-threads")) rc = int_arg(&i, argc, argv, 1, 255, "--max-threads", &o->max_threads);
        else if (IS("--tile-rows-log2")) rc = int_arg(&i, argc, argv, 0, 6, "--tile-rows-log2", &o->tile_rows_log2);
        else if (IS("--tile-cols-log2")) rc = int_arg(&i, argc, argv, 0, 6, "--tile-cols-log2", &o->tile_cols_log2);
        else if (IS("--auto-tiling")) rc = bool_arg(&i, argc, argv, "--auto-tiling", &o->auto_tiling);
        else if (IS("--tune")) {
            const char* t = arg_value(&i, argc, argv, "--tune");
            if (!t) return -1;
            if (strcmp(t, "ssim") && strcmp(t, "iq") && strcmp(t, "ssimulacra2")) {
                fprintf(stderr, "Error: --tune must be one of: ssim, iq, ssimulacra2\n");
                return fail("InvalidTuneMode", NULL);
            }
            o->tune = t;
        } else if (IS("--tenbit")) rc = bool_arg(&i, argc, argv, "--tenbit", &o->tenbit);
        else if (IS("--tolerance")) rc = float_arg(&i, argc, argv, 1, 100, "--tolerance", &o->tolerance);
        else if (IS("--max-pass")) rc = int_arg(&i, argc, argv, 1, 12, "--max-pass", &o->max_pass);
        else if (IS("-q") || IS("--quality")) rc = int_arg(&i, argc, argv, 0, 100, "--quality", &o->quality);
        else if (IS("--color-primaries")) rc = int_arg(&i, argc, argv, 1, 22, "--color-primaries", &o->color_primaries);
        else if (IS("--transfer-characteristics")) rc = int_arg(&i, argc, argv, 1, 18, "--transfer-characteristics", &o->transfer_characteristics);
        else if (IS("--matrix-coefficients")) rc = int_arg(&i, argc, argv, 0, 14, "--matrix-coefficients", &o->matrix_coefficients);
        else if (!*in) *in = a;
        else if (!*out) *out = a;
        else { fprintf(stderr, "Error: Unexpected argument: %s\n", a); return fail("UnexpectedArgument", NULL); }
#undef IS
        if (rc) return rc;
    }
    return 0;
}

/* ---- image load: io.zig's Image (io.zig:42-55) ------------------------------------------------------------ */
typedef struct {
    uint32_t w, h, channels; /* 3 or 4 after load (gray is expanded: see load_pam) */
    int hbd;                 /* data is u16, full 16-bit range */
    uint8_t* data;
    uint8_t* icc;
    size_t icc_len;
} Image;

static uint8_t* read_file(const char* path, size_t* len) {
    FILE* f = fopen(path, "rb");
    if (!f) { fail("FileNotFound", path); return NULL; }
    /* Read until end of file into a growing buffer: a FIFO or another non-seekable input named x.png has no size to
       ask for (ftell gives -1 there; ADVICE r04: that became malloc(1) + fread of SIZE_MAX bytes). */
    size_t cap = 1u << 16, n = 0;
    struct stat st;
    if (fstat(fileno(f), &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) cap = (size_t)st.st_size + 1;
    uint8_t* b = (uint8_t*)malloc(cap);
    while (b) {
        n += fread(b + n, 1, cap - n, f);
        if (n < cap) break; /* short read: end of file or an error */
        if (cap > SIZE_MAX / 2) { free(b); b = NULL; break; }
        uint8_t* g = (uint8_t*)realloc(b, cap * 2);
        if (!g) { free(b); b = NULL; break; }
        b = g;
        cap *= 2;
    }
    if (!b || ferror(f)) {
        fail(b ? "ReadFailed" : "OutOfMemory", path);
        fclose(f);
        free(b);
        return NULL;
    }
    fclose(f);
    *len = n;
    return b;
}

/* io.loadPAM (io.zig:309-406), the acceptance rules as oavif_amd/pam.py lists them: "P7"; the header ends at the
   first "ENDHDR\n", else at the first blank line; lines split on CR / LF, '#' comments, keys matched as prefixes,
   the first token after the key is the value; WIDTH, HEIGHT, DEPTH, MAXVAL all non-zero, MAXVAL 255, DEPTH 1..4;
   TUPLTYPE GRAYSCALE / GRAYSCALE_ALPHA / RGB / RGB_ALPHA must agree with DEPTH, BLACKANDWHITE is refused, anything
   else leaves DEPTH to decide; the raster must hold width*height*depth bytes.  Zig's error names. */
static const uint8_t* find_bytes(const uint8_t* b, size_t n, const char* pat) {
    const size_t m = strlen(pat);
    for (size_t i = 0; i + m <= n; ++i)
        if (memcmp(b + i, pat, m) == 0) return b + i;
    return NULL;
}
static int pam_value(const char* rest, char* tok, size_t cap) { /* first whitespace-separated token; 0 = none */
    while (*rest == ' ' || *rest == '\t') ++rest;
    size_t k = 0;
    while (*rest && *rest != ' ' && *rest != '\t' && k + 1 < cap) tok[k++] = *rest++;
    tok[k] = 0;
    return k > 0;
}
static int pam_usize(const char* tok, size_t* out) { /* std.fmt.parseInt(usize, tok, 10): digits, '_', a leading '+' */
    size_t v = 0;
    int digits = 0;
    if (*tok == '+') ++tok;
    for (; *tok; ++tok) {
        if (*tok == '_') continue;
        if (*tok < '0' || *tok > '9') return fail("InvalidCharacter", NULL);
        if (v > (SIZE_MAX - 9) / 10) return fail("Overflow", NULL);
        v = v * 10 + (size_t)(*tok - '0');
        digits = 1;
    }
    if (!digits) return fail("InvalidCharacter", NULL);
    *out = v;
    return 0;
}
static int load_pam(const uint8_t* b, size_t n, Image* im) {
    if (n < 3 || b[0] != 'P' || b[1] != '7') return fail("NotAPamFile", NULL);
    size_t header_end;
    const uint8_t* e = find_bytes(b, n, "ENDHDR\n");
    if (e) header_end = (size_t)(e - b) + 7;
    else if ((e = find_bytes(b, n, "\n\n")) != NULL) header_end = (size_t)(e - b) + 2;
    else return fail("HeaderNotFound", NULL);
    size_t w = 0, h = 0, depth = 0, maxval = 0;
    char tuple[64] = "UNSPECIFIED", tok[64];
    for (size_t p = 0; p < header_end;) {
        size_t q = p;
        while (q < header_end && b[q] != '\n' && b[q] != '\r') ++q;
        char line[160];
        const size_t L = q - p < sizeof line - 1 ? q - p : sizeof line - 1;
        memcpy(line, b + p, L);
        line[L] = 0;
        p = q + 1;
        if (!*line || *line == '#') continue;
        if (!strncmp(line, "WIDTH", 5)) { if (pam_value(line + 5, tok, sizeof tok) && pam_usize(tok, &w)) return -1; }
        else if (!strncmp(line, "HEIGHT", 6)) { if (pam_value(line + 6, tok, sizeof tok) && pam_usize(tok, &h)) return -1; }
        else if (!strncmp(line, "DEPTH", 5)) { if (pam_value(line + 5, tok, sizeof tok) && pam_usize(tok, &depth)) return -1; }
        else if (!strncmp(line, "MAXVAL", 6)) { if (pam_value(line + 6, tok, sizeof tok) && pam_usize(tok, &maxval)) return -1; }
        else if (!strncmp(line, "TUPLTYPE", 8)) { if (pam_value(line + 8, tok, sizeof tok)) snprintf(tuple, sizeof tuple, "%s", tok); }
        else if (!strcmp(line, "ENDHDR")) break;
    }
    if (!w || !h || !depth || !maxval) return fail("InvalidPamDimensions", NULL);
    if (maxval != 255) return fail("UnsupportedPamMaxVal", NULL);
    if (depth > 4) return fail("UnsupportedPamDepth", NULL);
    static const struct { const char* name; size_t ch; } kinds[] = {
        {"GRAYSCALE", 1}, {"GRAYSCALE_ALPHA", 2}, {"RGB", 3}, {"RGB_ALPHA", 4}};
    for (size_t k = 0; k < 4; ++k)
        if (!strcasecmp(tuple, kinds[k].name) && depth != kinds[k].ch) return fail("PamTupleMismatch", NULL);
    if (!strcasecmp(tuple, "BLACKANDWHITE")) return fail("UnsupportedPamTuple", NULL);
    if (w > 65536 || h > 65536) return fail("InsufficientDataInFile", NULL); /* no such raster fits the file anyway */
    const size_t px = w * h;
    if (px * depth > n - header_end) return fail("InsufficientDataInFile", NULL);
    /* gray (+alpha) is expanded to RGB(A): the reference hands 1- and 2-channel data to libavif as if it
       were RGB (io.zig:564), a row-stride bug this host does not reproduce */
    const uint32_t ch = depth <= 2 ? (uint32_t)depth + 2 : (uint32_t)depth;
    uint8_t* d = (uint8_t*)malloc(px * ch);
    if (!d) return fail("OutOfMemory", NULL);
    const uint8_t* s = b + header_end;
    for (size_t i = 0; i < px; ++i)
        for (uint32_t c = 0; c < ch; ++c)
            d[i * ch + c] = depth >= 3 ? s[i * depth + c] : (c < 3 ? s[i * depth] : s[i * depth + 1]);
    im->w = (uint32_t)w; im->h = (uint32_t)h; im->channels = ch; im->hbd = 0; im->data = d;
    return 0;
}

static int load_png(const uint8_t* b, size_t n, Image* im) { /* io.loadPNG (io.zig:242-307) via the C ABI */
    oavif_png_info info;
    int rc = oavif_png_info_from_memory(b, n, &info);
    if (rc) return fail(rc == OAVIF_PNG_ERR_HEADER ? "GetHeaderFailed" : rc == OAVIF_PNG_ERR_SIZE ? "ImageSizeFailed" : "DecodeFailed", NULL);
    uint8_t* d = (uint8_t*)malloc(info.data_bytes ? info.data_bytes : 1);
    uint8_t* icc = info.icc_bytes ? (uint8_t*)malloc(info.icc_bytes) : NULL;
    if (!d || (info.icc_bytes && !icc)) { free(d); free(icc); return fail("OutOfMemory", NULL); }
    rc = oavif_png_decode(b, n, d, info.data_bytes, icc, info.icc_bytes);
    if (rc) { free(d); free(icc); return fail("DecodeFailed", NULL); }
    im->w = info.width; im->h = info.height; im->channels = info.channels; im->hbd = info.hbd;
    im->data = d; im->icc = icc; im->icc_len = info.icc_bytes;
    return 0;
}

static int load_image(const char* path, Image* im) {
    const char* dot = strrchr(path, '.');
    size_t n = 0;
    if (!dot || (strcasecmp(dot, ".png") && strcasecmp(dot, ".pam"))) return fail("UnsupportedImageFormat", "this host reads PNG and PAM");
    uint8_t* b = read_file(path, &n);
    if (!b) return -1;
    const int rc = strcasecmp(dot, ".png") == 0 ? load_png(b, n, im) : load_pam(b, n, im);
    free(b);
    return rc;
}

/* ---- the pass: io.encodeAvifToBuffer + decodeAvifCommon + the score (tq.zig:21-38) ------------------------- */
typedef struct { /* what every pass encodes: filled once, then only read (the probes of a wave share it on threads) */
    const Options* o;
    const Image* src;
    const void* scaled;   /* the source at the encoder's depth, computed once */
    uint32_t out_depth;
    avifImageHead* image; /* ... and as the encoder takes it (YUV444), converted once: make_source_image() */
} Source;

/* io.zig:550-623, hoisted out of the pass loop: the avifImage of the source -- created, tagged (CICP, ICC) and
   converted to YUV444 -- is made ONCE.  The reference rebuilds it on every pass (avifImageCreate +
   avifImageRGBToYUV over the whole frame, 15 % of a 4K encode at speed 9) although only `quality` changes between
   passes (io.zig:625).  Same planes, same bitstream. */
static int make_source_image(Source* e) {
    const Options* o = e->o;
    const Image* s = e->src;
    int r;
    avifImageHead* image = av.ImageCreate(s->w, s->h, e->out_depth, AVIF_YUV444);
    if (!image) return fail("OutOfMemory", NULL);
    image->colorPrimaries = (uint16_t)o->color_primaries;
    image->transferCharacteristics = (uint16_t)o->transfer_characteristics;
    image->matrixCoefficients = (uint16_t)o->matrix_coefficients;
    if (s->icc && av.ImageSetProfileICC(image, s->icc, s->icc_len) != AVIF_OK) {
        av.ImageDestroy(image);
        return fail("SetICCProfileFailed", NULL);
    }
    avifRGBImage rgb;
    memset(&rgb, 0, sizeof rgb);
    av.RGBImageSetDefaults(&rgb, image);
    rgb.format = s->channels == 4 ? AVIF_RGBA : AVIF_RGB;
    rgb.pixels = (uint8_t*)(uintptr_t)e->scaled;
    rgb.rowBytes = s->w * s->channels * (e->out_depth > 8 ? 2u : 1u);
    rgb.depth = e->out_depth;
    if ((r = av.ImageRGBToYUV(image, &rgb)) != AVIF_OK) {
        av.ImageDestroy(image);
        return fail("ConvertFailed", av.ResultToString(r));
    }
    e->image = image;
    return 0;
}

static int encode_to_buffer(const Source* e, uint32_t q, uint8_t** out, size_t* out_size) { /* io.zig:619-635 */
    const Options* o = e->o;
    avifEncoderHead* enc = NULL;
    avifRWData output = {NULL, 0};
    int rc = -1, r;
    enc = av.EncoderCreate();
    if (!enc) { fail("OutOfMemory", NULL); goto done; }
    enc->qualityAlpha = o->quality_alpha; /* copyToEncoder (parse_args.zig:65-74) */
    enc->speed = o->speed;
    enc->maxThreads = o->max_threads;
    enc->tileRowsLog2 = o->tile_rows_log2;
    enc->tileColsLog2 = o->tile_cols_log2;
    enc->autoTiling = o->auto_tiling;
    if (av.EncoderSetCodecSpecificOption(enc, "tune", o->tune) != AVIF_OK) { fail("InvalidCodecOption", NULL); goto done; }
    enc->quality = (int)q; /* io.zig:625-626 */
    enc->qualityAlpha = o->quality_alpha;
    if ((r = av.EncoderAddImage(enc, e->image, 1, AVIF_ADD_IMAGE_FLAG_SINGLE)) != AVIF_OK) { fail("AddImageFailed", av.ResultToString(r)); goto done; }
    if ((r = av.EncoderFinish(enc, &output)) != AVIF_OK) { fail("FinishFailed", av.ResultToString(r)); goto done; }
    *out = (uint8_t*)malloc(output.size);
    if (!*out) { fail("OutOfMemory", NULL); goto done; }
    memcpy(*out, output.data, output.size);
    *out_size = output.size;
    rc = 0;
done:
    if (output.data) av.RWDataFree(&output);
    if (enc) av.EncoderDestroy(enc);
    return rc;
}

/* io.zig:546: can the loaded libavif write 10-bit?  A libaom without high-bit-depth support cannot; asked once, with
   a 16x16 gray image at speed 10 and the run's other options. */
static int supports_10bit(const Options* o) {
    Options po = *o;
    po.speed = 10;
    uint16_t tiny[16 * 16 * 3];
    for (int i = 0; i < 16 * 16 * 3; ++i) tiny[i] = 512;
    const Image ti = {16, 16, 3, 0, (uint8_t*)tiny, NULL, 0};
    Source s = {&po, &ti, tiny, 10, NULL};
    uint8_t* b = NULL;
    size_t n = 0;
    const int refused = make_source_image(&s) || encode_to_buffer(&s, 50, &b, &n);
    if (s.image) av.ImageDestroy(s.image);
    free(b);
    forget_failure();
    return !refused;
}

/* One pass (computeScoreAtQuality, tq.zig:21-38) in two halves: the CPU half (encode at q, decode to libavif's
   8-bit RGB(A) rows) touches nothing shared but the read-only source, so the probes of a speculative wave
   run it on threads and the FIRST pass of a run runs it while the scorer is still starting up; the GPU half
   scores those rows on a given context. */
typedef struct { avifDecoderHead* dec; avifRGBImage rgb; int caller_pixels; } Decoded;
static void decoded_free(Decoded* d) {
    if (d->rgb.pixels && !d->caller_pixels) av.RGBImageFreePixels(&d->rgb);
    if (d->dec) av.DecoderDestroy(d->dec);
    memset(d, 0, sizeof *d);
}
static int pass_cpu(const Source* e, uint32_t q, uint8_t** out_avif, size_t* out_size, Decoded* d, double times_ms[3],
                    uint8_t* pinned) {
    uint8_t* avif = NULL;
    size_t avif_size = 0;
    memset(d, 0, sizeof *d);
    double t0 = now_ms();
    if (encode_to_buffer(e, q, &avif, &avif_size)) return -1;
    double t1 = now_ms();
    /* decodeAvifCommon(avif, use_8bit = true) (io.zig:452-482) */
    int rc = -1, r;
    d->dec = av.DecoderCreate();
    if (!d->dec) { fail("OutOfMemory", NULL); goto done; }
    if (av.DecoderSetIOMemory(d->dec, avif, avif_size) != AVIF_OK) { fail("SetIOFailed", NULL); goto done; }
    if ((r = av.DecoderParse(d->dec)) != AVIF_OK) { fail("ParseFailed", av.ResultToString(r)); goto done; }
    if ((r = av.DecoderNextImage(d->dec)) != AVIF_OK) { fail("DecodeImageFailed", av.ResultToString(r)); goto done; }
    const avifImageHead* img = d->dec->image;
    if (!img || img->width != e->src->w || img->height != e->src->h) { fail("DecodeImageFailed", "unexpected frame size"); goto done; }
    av.RGBImageSetDefaults(&d->rgb, img);
    d->rgb.depth = 8;                                        /* io.zig:470-471 */
    d->rgb.format = img->alphaPlane ? AVIF_RGBA : AVIF_RGB;  /* io.zig:473 */
    if (pinned) { /* the caller's buffer in place of avifRGBImageAllocatePixels: tight rows, as libavif would lay them */
        d->rgb.pixels = pinned;
        d->rgb.rowBytes = img->width * (d->rgb.format == AVIF_RGBA ? 4u : 3u);
        d->caller_pixels = 1;
    } else if (av.RGBImageAllocatePixels(&d->rgb) != AVIF_OK) { fail("AllocatePixelsFailed", NULL); goto done; }
    if ((r = av.ImageYUVToRGB(img, &d->rgb)) != AVIF_OK) { fail("ConvertToRGBFailed", av.ResultToString(r)); goto done; }
    times_ms[0] = t1 - t0; times_ms[1] = now_ms() - t1;
    *out_avif = avif; *out_size = avif_size;
    avif = NULL;
    rc = 0;
done:
    if (rc) decoded_free(d);
    free(avif);
    return rc;
}
static int pass_score(ssimu2_ctx* scorer, Decoded* d, double* out_score, double times_ms[3]) {
    /* tq.zig:37, without the copy loop of io.zig:654-663: libavif's rows as they are */
    const double t = now_ms();
    const int r = ssimu2_score_against_reference_strided(scorer, d->rgb.pixels, d->rgb.rowBytes,
                                                         d->rgb.format == AVIF_RGBA ? 4 : 3, out_score);
    times_ms[2] = now_ms() - t;
    decoded_free(d);
    return r == SSIMU2_OK ? 0 : fail("ScorerFailed", ssimu2_last_error(scorer));
}

/* ---- the run: everything it allocates, released on every path (run_free) -------------------------------------- */
/* One scorer context (= one HIP stream + scratch) and what a probe on it needs.  `pinned` is decodeAvifCommon's RGB
   buffer (io.zig:452-482) in page-locked memory of the scorer (ssimu2_host_alloc): libavif converts straight into it
   and the upload is one DMA.  NULL = libavif's own buffer: the context is not up yet, OAVIF_HOST_PINNED=0, or the
   allocation failed (not fatal, tried once).  With OAVIF_SCORER_SOCKET set (a scoring service, include/ssimu2_hip.h)
   nothing here changes: the same call returns memory the service maps, and it reads the frame where libavif wrote it.
   A sequential search uses slot 0; a wave of a fanned one runs probe i on slot i, one thread per slot at a time. */
typedef struct { ssimu2_ctx* ctx; int ready /* blur and reference set */; uint8_t* pinned; int pinned_tried; } Slot;

typedef struct {
    Env env;
    double t0;
    Options o;
    Image src;
    uint8_t* rgb8; /* e.rgb: the scorer's reference */
    void* scaled;
    const char* depth_note;
    Source source;
    Slot slots[OAVIF_TQ_MAX_FANOUT]; /* the only owner of scorer contexts and page-locked frame buffers */
    /* EncBuffer (main.zig:11-19) for every probe, not the last one only: any may be the answer.  Under g_lock. */
    struct { uint32_t q; uint8_t* b; size_t n; } kept[OAVIF_TQ_MAX_PASS * OAVIF_TQ_MAX_FANOUT];
    int nkept;
    double encode_ms, decode_ms, score_ms; /* summed over the probes, under g_lock */
    uint8_t* encoded; /* the bytes of -q, or of a chosen q that no probe encoded */
} Run;

static void phase(const Run* r, const char* what) { /* OAVIF_HOST_TIMES: where a one-image run spends its wall time */
    if (r->env.times) fprintf(stderr, "  [%7.1f ms] %s\n", now_ms() - r->t0, what);
}

static int slot_create(Run* r, Slot* s) { /* ssimu2_prefetch started the runtime at process start; this waits for it */
    if (s->ctx) return 0;
    const int rc = ssimu2_ctx_create(r->env.device, NULL, &s->ctx);
    if (rc != SSIMU2_OK)
        return fail(rc == SSIMU2_ERR_NO_DEVICE && s == r->slots ? "NoDevice" : "ScorerFailed", ssimu2_last_error(NULL));
    if (s == r->slots) phase(r, "scorer context created");
    return 0;
}
static int slot_prepare(Run* r, Slot* s) { /* the context, blur and reference set, the page-locked buffer tried: each once */
    if (slot_create(r, s)) return -1;
    if (!s->ready) {
        if (ssimu2_ctx_set_blur(s->ctx, r->env.blur) || ssimu2_set_reference(s->ctx, r->rgb8, r->src.w, r->src.h))
            return fail("ScorerFailed", ssimu2_last_error(s->ctx));
        s->ready = 1;
        if (s == r->slots) phase(r, "reference uploaded and cached");
    }
    if (!s->pinned_tried) {
        void* p = NULL; /* room for RGBA rows */
        s->pinned_tried = 1;
        if (r->env.pinned && ssimu2_host_alloc(s->ctx, (size_t)r->src.w * r->src.h * 4, &p) == SSIMU2_OK) s->pinned = (uint8_t*)p;
    }
    return 0;
}
static void slot_release(Slot* s) {
    if (!s->ctx) return;
    ssimu2_host_free(s->ctx, s->pinned);
    ssimu2_ctx_destroy(s->ctx);
    memset(s, 0, sizeof *s);
}

static void run_free(Run* r) {
    for (uint32_t i = 0; i < OAVIF_TQ_MAX_FANOUT; ++i) slot_release(&r->slots[i]);
    for (int k = 0; k < r->nkept; ++k) free(r->kept[k].b);
    if (r->source.image) av.ImageDestroy(r->source.image);
    free(r->encoded);
    if (r->scaled != r->src.data) free(r->scaled);
    if (r->rgb8 != r->src.data) free(r->rgb8);
    free(r->src.data);
    free(r->src.icc);
}

/* The pass of both searches: probe q on a slot and keep its bytes.  A slot whose context exists is prepared before
   the CPU half, so that the frame is decoded into its page-locked buffer.  Slot 0 of a sequential search has none at
   its first probe: the scorer's start-up (0.1-0.25 s, begun by ssimu2_prefetch) runs behind that probe's CPU half --
   its quantizer does not depend on any score (tq.zig:136) -- and the context is made when the score needs it. */
static int run_probe(Run* r, uint32_t slot, uint32_t q, double* out_score) {
    Slot* s = &r->slots[slot];
    uint8_t* avif = NULL;
    size_t n = 0;
    double t[3] = {0, 0, 0};
    Decoded d;
    if (s->ctx && slot_prepare(r, s)) return -1;
    if (pass_cpu(&r->source, q, &avif, &n, &d, t, s->pinned)) return -1;
    if (!s->ctx) phase(r, "first probe encoded and decoded");
    if (slot_prepare(r, s) || pass_score(s->ctx, &d, out_score, t)) { decoded_free(&d); free(avif); return -1; }
    pthread_mutex_lock(&g_lock);
    r->encode_ms += t[0]; r->decode_ms += t[1]; r->score_ms += t[2];
    if (r->nkept < (int)(sizeof r->kept / sizeof r->kept[0])) {
        r->kept[r->nkept].q = q; r->kept[r->nkept].b = avif; r->kept[r->nkept].n = n;
        ++r->nkept;
        avif = NULL;
    }
    pthread_mutex_unlock(&g_lock);
    free(avif);
    return 0;
}
static int probe_one(void* user, uint32_t q, double* out_score) { return run_probe((Run*)user, 0, q, out_score); }

/* ---- the probes of one search fanned over scorer contexts and host threads (BASELINE
   configs[2]): oavif_tq_find_target_quality_speculative asks for waves of quantizers, each probe of a wave runs
   the pass above on its own slot and thread.  OAVIF_PROBE_FANOUT=N, as the Python mirror; the result is the
   sequential search's (include/oavif_tq.h). ------------------------------------------------------------------ */
typedef struct { Run* r; uint32_t slot, q; double score; int rc; } Job;
static void* job_run(void* arg) {
    Job* j = (Job*)arg;
    j->rc = run_probe(j->r, j->slot, j->q, &j->score);
    return NULL;
}
static int probe_wave(void* user, const uint32_t* qs, uint32_t n, double* out_scores) {
    Run* r = (Run*)user;
    Job jobs[OAVIF_TQ_MAX_FANOUT];
    pthread_t th[OAVIF_TQ_MAX_FANOUT];
    int started[OAVIF_TQ_MAX_FANOUT] = {0};
    if (n > (uint32_t)r->env.fanout) return fail("SearchFailed", "wave larger than the fan-out");
    for (uint32_t i = 0; i < n; ++i) {
        jobs[i].r = r; jobs[i].slot = i; jobs[i].q = qs[i]; jobs[i].score = 0; jobs[i].rc = -1;
        if (i + 1 == n) job_run(&jobs[i]); /* the last probe of a wave runs on the calling thread */
        else started[i] = pthread_create(&th[i], NULL, job_run, &jobs[i]) == 0;
        if (i + 1 < n && !started[i]) job_run(&jobs[i]);
    }
    int rc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (started[i]) pthread_join(th[i], NULL);
        if (jobs[i].rc) rc = -1;
        out_scores[i] = jobs[i].score;
    }
    return rc;
}

/* ---- the phases of a run (main.zig:73-116) ------------------------------------------------------------------ */
static int load_source(Run* r, const char* in) { /* main.zig:73-91: the image and the scorer's RGB8 reference */
    Image* src = &r->src;
    if (load_image(in, src)) return -1;
    phase(r, "image loaded");
    struct stat st;
    memset(&st, 0, sizeof st);
    stat(in, &st);
    fprintf(stderr, "Read %ux%u, %s, %d-bit, %lld bytes\n", src->w, src->h, src->channels > 3 ? "RGBA" : "RGB",
            src->hbd ? 16 : 8, (long long)st.st_size);
    /* e.rgb: Image.toRGB8 (io.zig:57-133) unless the source already is RGB8 (main.zig:86) */
    const size_t px = (size_t)src->w * src->h;
    r->rgb8 = src->data;
    if (src->channels != 3 || src->hbd) {
        r->rgb8 = (uint8_t*)malloc(px * 3);
        if (!r->rgb8) return fail("OutOfMemory", NULL);
        for (size_t i = 0; i < px; ++i)
            for (int c = 0; c < 3; ++c)
                r->rgb8[i * 3 + c] = src->hbd ? (uint8_t)(((const uint16_t*)src->data)[i * src->channels + c] >> 8)
                                              : src->data[i * src->channels + c];
    }
    return 0;
}

/* The encoder's depth (io.zig:546) and the source rescaled to it (io.zig:566-617), hoisted out of the pass loop
   (SURVEY.md 8f rank 4); r->source describes the result, its avifImage still to be made. */
static int scale_source(Run* r) {
    const Image* src = &r->src;
    const size_t nsamp = (size_t)src->w * src->h * src->channels;
    uint32_t out_depth = (r->o.tenbit || src->hbd) ? 10 : 8;
    if (out_depth == 10 && !supports_10bit(&r->o)) {
        out_depth = 8;
        r->depth_note = "note: the reference would write 10-bit here (--tenbit 1 / 16-bit source, io.zig:546-548); this "
                        "image's libaom has no high-bit-depth support, so the bitstream is 8-bit";
    }
    r->scaled = src->data;
    if (src->hbd || out_depth == 10) {
        r->scaled = malloc(nsamp * (out_depth == 10 ? 2 : 1));
        if (!r->scaled) return fail("OutOfMemory", NULL);
        if (!src->hbd) oavif_prescale_8_to_10(src->data, nsamp, (uint16_t*)r->scaled);
        else if (out_depth == 10) oavif_prescale_16_to_10((const uint16_t*)src->data, nsamp, (uint16_t*)r->scaled);
        else oavif_prescale_16_to_8((const uint16_t*)src->data, nsamp, (uint8_t*)r->scaled);
    }
    r->source = (Source){&r->o, src, r->scaled, out_depth, NULL};
    return 0;
}

static int write_file(const char* path, const uint8_t* b, size_t n) {
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(b, 1, n, f) != n) { if (f) fclose(f); return fail("WriteFailed", path); }
    fclose(f);
    return 0;
}
static int write_output(const Run* r, const char* out, const uint8_t* b, size_t n) {
    if (write_file(out, b, n)) return -1;
    fprintf(stderr, "Compressed to %zu bytes (%.3f bpp)\n", n, n * 8.0 / ((double)r->src.w * r->src.h));
    if (r->depth_note) fprintf(stderr, "%s\n", r->depth_note);
    return 0;
}

static int encode_once(Run* r, const char* out) { /* -q, main.zig:93-100 */
    size_t n = 0;
    fprintf(stderr, "Encoding [q%d, speed %d, %u-bit]\n", r->o.quality, r->o.speed, r->source.out_depth);
    if (make_source_image(&r->source) || encode_to_buffer(&r->source, (uint32_t)r->o.quality, &r->encoded, &n)) return -1;
    return write_output(r, out, r->encoded, n);
}

static int search(Run* r, const char* out) { /* main.zig:102-116 */
    const Options* o = &r->o;
    if (o->score_tgt == floor(o->score_tgt)) /* Zig's {} on an f64 prints 80 for 80.0 */
        fprintf(stderr, "Searching [tgt %.0f±%.1f, speed %d, %u-bit]\n", o->score_tgt, o->tolerance, o->speed, r->source.out_depth);
    else
        fprintf(stderr, "Searching [tgt %g±%.1f, speed %d, %u-bit]\n", o->score_tgt, o->tolerance, o->speed, r->source.out_depth);
    if (make_source_image(&r->source)) return -1; /* before the first wave: the threads only read it */
    phase(r, "source converted to YUV444");
    const oavif_tq_options to = {o->score_tgt, o->tolerance, (uint32_t)o->max_pass};
    oavif_tq_result res;
    oavif_tq_spec_stats stats = {0, 0, 0};
    const int fanned = r->env.fanout > 1;
    int rc;
    if (fanned) { /* its contexts up front, made here on one thread; the reference goes to slot i when a wave first uses it */
        if (slot_prepare(r, &r->slots[0])) return -1;
        for (int i = 1; i < r->env.fanout; ++i)
            if (slot_create(r, &r->slots[i])) return -1;
        const oavif_tq_spec_options so = OAVIF_TQ_SPEC_OPTIONS_INIT((uint32_t)r->env.fanout, 1);
        rc = oavif_tq_find_target_quality_speculative(&to, &so, probe_wave, r, &res, &stats);
    } else {
        rc = oavif_tq_find_target_quality(&to, probe_one, r, &res);
    }
    if (rc) return g_err ? -1 : fail("SearchFailed", NULL);
    phase(r, "search done");
    fprintf(stderr, "Found q%u (score %.2f, %u passes)\n", res.q, res.score, res.num_pass);
    int k = 0; /* main.zig:109-113: the bytes of the chosen q if a probe encoded it, else one more encode */
    while (k < r->nkept && r->kept[k].q != res.q) ++k;
    if (k < r->nkept) {
        if (write_output(r, out, r->kept[k].b, r->kept[k].n)) return -1;
    } else {
        size_t n = 0;
        if (encode_to_buffer(&r->source, res.q, &r->encoded, &n) || write_output(r, out, r->encoded, n)) return -1;
    }
    if (r->env.times && fanned)
        fprintf(stderr, "speculative: %u waves, %u probes issued, %u cache hits\n", stats.waves, stats.probes_issued,
                stats.cache_hits);
    if (r->env.times) /* not one of the reference's lines: only on request */
        fprintf(stderr, "times: encode %.1f ms, decode %.1f ms, upload+score %.2f ms over %u passes\n", r->encode_ms,
                r->decode_ms, r->score_ms, res.num_pass);
    return 0;
}

static int run_inner(Run* r, int argc, char** argv) {
    const char *in = NULL, *out = NULL;
    r->o = (Options)OPTIONS_DEFAULT;
    if (parse_args(&r->o, argc, argv, &in, &out)) return -1;
    if (!in || !out) return fail("MissingInputOrOutput", NULL);
    if (r->o.quality < 0) ssimu2_prefetch(r->env.device); /* the HIP start-up runs behind the image load and the first encode */
    phase(r, "arguments parsed, scorer start-up begun in the background");
    if (load_libavif(r->env.libavif)) return -1;
    phase(r, "libavif opened and checked");
    if (load_source(r, in) || scale_source(r)) return -1;
    return r->o.quality >= 0 ? encode_once(r, out) : search(r, out);
}

static int run(int argc, char** argv) {
    Run r;
    memset(&r, 0, sizeof r);
    r.t0 = now_ms();
    env_read(&r.env);
    const int rc = run_inner(&r, argc, argv);
    phase(&r, "output written");
    run_free(&r);
    phase(&r, "contexts and buffers released");
    return rc;
}

/* parse_args.zig:180-238: the usage text with the defaults of the options struct filled in */
static void print_usage(void) {
    const Options d = OPTIONS_DEFAULT;
    fprintf(stderr,
            "\nusage:  oavif [options] <in> <out.avif>\n\noptions:\n"
            " -h, --help\n    show this help\n"
            " -v, --version\n    show version information\n"
            " -s, --speed u8\n    encoder speed (0..10) [%d]\n"
            " -t, --score-tgt f64\n    target SSIMULACRA2 score (0..100) [%.0f]\n"
            " --quality-alpha u8\n    quality factor for alpha (0..100=lossless) [%d]\n"
            " --max-threads u8\n    maximum number of threads to use (1..255) [%d]\n"
            " --tile-rows-log2 u8\n    tile rows log2 (0..6) [%d]\n"
            " --tile-cols-log2 u8\n    tile columns log2 (0..6) [%d]\n"
            " --auto-tiling 0/1\n    enable automatic tiling [%d]\n"
            " --tune str\n    libaom tuning mode (ssim, iq, ssimulacra2) [%s]\n"
            " --tenbit 0/1\n    force 10-bit AVIF output [%d]\n"
            " --tolerance f64\n    target quality error tolerance (1..100) [%.0f]\n"
            " --max-pass u8\n    maximum search passes (1..12) [%d]\n"
            " -q, --quality u8\n    quantizer (0..100), bypasses search\n"
            " --color-primaries u8\n    color primaries (1..22) [%d]\n"
            " --transfer-characteristics u8\n    transfer characteristics (1..18) [%d]\n"
            " --matrix-coefficients u8\n    matrix coefficients (0..14) [%d]"
            "\n\n\x1b[37mInput image formats: PNG, PAM, JPEG, WebP, or AVIF\x1b[0m\n",
            d.speed, d.score_tgt, d.quality_alpha, d.max_threads, d.tile_rows_log2, d.tile_cols_log2, d.auto_tiling, d.tune,
            d.tenbit, d.tolerance, d.max_pass, d.color_primaries, d.transfer_characteristics, d.matrix_coefficients);
}

/* io.printVersion (io.zig:14-39) for what this host links: itself, the scorer library, libavif and its codecs */
static void print_version(void) {
    fprintf(stderr, "oavif %s\nscorer %s\n", VERSION, ssimu2_version());
    Env env;
    env_read(&env);
    if (load_libavif(env.libavif) == 0) fprintf(stderr, "libavif %s\n", av.Version());
}

int main(int argc, char** argv) {
    fprintf(stderr, "\x1b[31moavif\x1b[0m | %s\n", VERSION);
    /* main.zig:46-61: -h/--help and -v/--version count only while they are the leading arguments */
    int show_help = 0, show_version = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) show_help = 1;
        else if (!strcmp(argv[i], "--version") || !strcmp(argv[i], "-v")) show_version = 1;
        else break;
    }
    if (show_help) { print_usage(); return 0; }
    if (show_version) { print_version(); return 0; }
    int rc = 0;
    if (run(argc, argv)) {
        fprintf(stderr, "error: %s%s%s\n", g_err ? g_err : "Unexpected", g_detail[0] ? ": " : "", g_detail);
        rc = 1;
    }
    /* Everything this process owns is released and its output is on disk.  The HIP runtime's exit handlers then
       spend another 50-100 ms unloading code objects and tearing the device context down -- a third of a 1080p
       run -- for memory the kernel reclaims anyway: leave without them (OAVIF_HOST_ATEXIT=1 keeps them, for
       leak checkers). */
    fflush(NULL);
    if (!getenv("OAVIF_HOST_ATEXIT")) _exit(rc);
    return rc;
}
