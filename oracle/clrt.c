/*
 * clrt.c -- a CPU work-item runtime for the reference's three OpenCL C kernels (TEST INFRASTRUCTURE ONLY).
 *
 * oracle/build_ref.py extracts nvf.hpp, me_p3.hpp and scaled_neighbors_p3.hpp from a reference checkout, compiles them
 * as OpenCL C for x86-64 with clang, and links them with this file into oracle/_ref/libwm_ref.so.  The objects call a
 * handful of OpenCL built-ins; this file defines them with the same mangled names and the x86-64 psABI's vector
 * passing (float4 / int2 in an XMM register, float8 in a YMM register: built with the kernels' -m flags):
 *   get_global_id / get_local_id / get_group_id / get_local_size / get_global_size,
 *   get_image_width / get_image_height, read_imagef(image2d_ro, sampler, int2), __translate_sampler_initializer,
 *   barrier, vstore_half4 / vstore_half8 (to local memory).
 *
 * Execution model: one work-group at a time per OpenMP thread (OMP_NUM_THREADS applies); inside a group one fiber
 * (ucontext) per work-item, so barrier() really suspends the work-item until every work-item of the group has reached
 * it.  Work-items of one group that disagree on their barrier count abort the process with a message.
 * Local memory is filled with 0xff bytes (a NaN in f32 and f16) before each group, so a read of a location no
 * work-item wrote shows up in the output.
 *
 * Images reproduce the reference's transposed layout (Watermark.cpp:57: an image of width = rows, height = cols,
 * filled from ArrayFire's column-major plane): get_image_width = rows, get_image_height = cols, and texel (u, v) is
 * x[clamp(u)][clamp(v)] of a row-major plane.  The only sampler accepted is the kernels' unnormalised
 * CLAMP_TO_EDGE | NEAREST one; any other aborts.
 */
#include <immintrin.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ucontext.h>

typedef float float4 __attribute__((vector_size(16)));
typedef float float8 __attribute__((vector_size(32)));
typedef int int2 __attribute__((vector_size(8)));

#define ALIGN_UP(v, a) ((((v) + (a) - 1) / (a)) * (a))
#define SAMPLER_KERNELS 0x12 /* CLK_NORMALIZED_COORDS_FALSE | CLK_ADDRESS_CLAMP_TO_EDGE | CLK_FILTER_NEAREST */
#define FIBER_STACK (64 * 1024)
#define MAX_ITEMS 256

typedef struct { const float* x; int rows, cols; } clrt_image;
typedef struct { int value; } clrt_sampler;

enum { RUNNING = 0, AT_BARRIER = 1, DONE = 2 };

typedef struct {
    ucontext_t ctx;
    size_t lid[2];
    int barriers, state;
} clrt_item;

typedef struct {
    size_t gid[2], lsz[2], gsz[2];
    int n, cur;
    void (*body)(void* arg, void* local);
    void* arg;
    void* local;
    ucontext_t sched;
    clrt_item items[MAX_ITEMS];
    char* stacks;
} clrt_group;

static _Thread_local clrt_group* tg;

static void die(const char* msg)
{
    fprintf(stderr, "wm_ref runtime: %s\n", msg);
    abort();
}

/* ---- work-item functions (OpenCL 1.2 6.12.1) ---- */
size_t get_global_id(unsigned d) __asm__("_Z13get_global_idj");
size_t get_local_id(unsigned d) __asm__("_Z12get_local_idj");
size_t get_group_id(unsigned d) __asm__("_Z12get_group_idj");
size_t get_local_size(unsigned d) __asm__("_Z14get_local_sizej");
size_t get_global_size(unsigned d) __asm__("_Z15get_global_sizej");
size_t get_global_id(unsigned d) { return d < 2 ? tg->gid[d] * tg->lsz[d] + tg->items[tg->cur].lid[d] : 0; }
size_t get_local_id(unsigned d) { return d < 2 ? tg->items[tg->cur].lid[d] : 0; }
size_t get_group_id(unsigned d) { return d < 2 ? tg->gid[d] : 0; }
size_t get_local_size(unsigned d) { return d < 2 ? tg->lsz[d] : 1; }
size_t get_global_size(unsigned d) { return d < 2 ? tg->gsz[d] : 1; }

void barrier(unsigned flags) __asm__("_Z7barrierj");
void barrier(unsigned flags)
{
    (void)flags;
    clrt_item* it = &tg->items[tg->cur];
    it->barriers++;
    it->state = AT_BARRIER;
    if (swapcontext(&it->ctx, &tg->sched) != 0) die("swapcontext failed");
}

/* ---- images and samplers ---- */
int get_image_width(const clrt_image* im) __asm__("_Z15get_image_width14ocl_image2d_ro");
int get_image_height(const clrt_image* im) __asm__("_Z16get_image_height14ocl_image2d_ro");
int get_image_width(const clrt_image* im) { return im->rows; }
int get_image_height(const clrt_image* im) { return im->cols; }

static const clrt_sampler kernel_sampler = {SAMPLER_KERNELS};

const clrt_sampler* __translate_sampler_initializer(int value)
{
    if (value != SAMPLER_KERNELS) die("sampler other than unnormalised CLAMP_TO_EDGE | NEAREST");
    return &kernel_sampler;
}

static inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

float4 read_imagef(const clrt_image* im, const clrt_sampler* s, int2 uv) __asm__("_Z11read_imagef14ocl_image2d_ro11ocl_samplerDv2_i");
float4 read_imagef(const clrt_image* im, const clrt_sampler* s, int2 uv)
{
    if (s != &kernel_sampler || s->value != SAMPLER_KERNELS) die("unknown sampler");
    const float l = im->x[(size_t)clampi(uv[0], im->rows - 1) * im->cols + clampi(uv[1], im->cols - 1)];
    return (float4){l, l, l, 1.0f}; /* CL_LUMINANCE: (L, L, L, 1) */
}

/* ---- vstore_half: f32 -> f16 round to nearest even (F16C, explicit rounding mode) ---- */
#define F32_TO_F16(f) _cvtss_sh((f), _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC)
void vstore_half4(float4 v, size_t off, uint16_t* p) __asm__("_Z12vstore_half4Dv4_fmPU7CLlocalDh");
void vstore_half8(float8 v, size_t off, uint16_t* p) __asm__("_Z12vstore_half8Dv8_fmPU7CLlocalDh");
void vstore_half4(float4 v, size_t off, uint16_t* p)
{
    for (int i = 0; i < 4; i++) p[off * 4 + i] = F32_TO_F16(v[i]);
}
void vstore_half8(float8 v, size_t off, uint16_t* p)
{
    for (int i = 0; i < 8; i++) p[off * 8 + i] = F32_TO_F16(v[i]);
}

/* ---- groups of fibers ---- */
static void fiber_main(void)
{
    tg->body(tg->arg, tg->local);
    tg->items[tg->cur].state = DONE;
    /* returning resumes uc_link = the scheduler */
}

static void run_group(clrt_group* g)
{
    for (int i = 0; i < g->n; i++) {
        clrt_item* it = &g->items[i];
        it->lid[0] = (size_t)i % g->lsz[0];
        it->lid[1] = (size_t)i / g->lsz[0];
        it->barriers = 0;
        it->state = RUNNING;
        if (getcontext(&it->ctx) != 0) die("getcontext failed");
        it->ctx.uc_stack.ss_sp = g->stacks + (size_t)i * FIBER_STACK;
        it->ctx.uc_stack.ss_size = FIBER_STACK;
        it->ctx.uc_link = &g->sched;
        makecontext(&it->ctx, fiber_main, 0);
    }
    for (;;) {
        for (int i = 0; i < g->n; i++) {
            if (g->items[i].state == DONE) continue;
            g->items[i].state = RUNNING;
            g->cur = i;
            if (swapcontext(&g->sched, &g->items[i].ctx) != 0) die("swapcontext failed");
        }
        int done = 0;
        for (int i = 0; i < g->n; i++) {
            done += g->items[i].state == DONE;
            if (g->items[i].barriers != g->items[0].barriers)
                die("work-items of one work-group disagree on the number of barriers");
        }
        if (done == g->n) return;
        if (done != 0) die("some work-items of a work-group returned while others wait at a barrier");
    }
}

/* NDRange (gsz0, gsz1) in groups of (lsz0, lsz1); both global sizes are multiples of the local sizes (OpenCL 1.2) */
static int launch(size_t gsz0, size_t gsz1, size_t lsz0, size_t lsz1, size_t local_bytes,
                  void (*body)(void*, void*), void* arg)
{
    if (gsz0 % lsz0 || gsz1 % lsz1 || lsz0 * lsz1 > MAX_ITEMS) return -1;
    const long ng0 = (long)(gsz0 / lsz0), ngroups = ng0 * (long)(gsz1 / lsz1);
    int failed = 0;
#pragma omp parallel
    {
        clrt_group* g = (clrt_group*)calloc(1, sizeof(clrt_group));
        char* stacks = g ? (char*)aligned_alloc(64, (size_t)MAX_ITEMS * FIBER_STACK) : NULL;
        void* local = g ? aligned_alloc(64, ALIGN_UP(local_bytes, 64)) : NULL;
        if (!g || !stacks || !local) {
#pragma omp atomic write
            failed = 1;
        } else {
            g->lsz[0] = lsz0; g->lsz[1] = lsz1;
            g->gsz[0] = gsz0; g->gsz[1] = gsz1;
            g->n = (int)(lsz0 * lsz1);
            g->body = body; g->arg = arg; g->local = local; g->stacks = stacks;
            tg = g;
#pragma omp for schedule(dynamic, 4)
            for (long k = 0; k < ngroups; k++) {
                g->gid[0] = (size_t)(k % ng0);
                g->gid[1] = (size_t)(k / ng0);
                memset(local, 0xff, local_bytes);
                run_group(g);
            }
            tg = NULL;
        }
        free(local);
        free(stacks);
        free(g);
    }
    return failed ? -1 : 0;
}

/* ---- the kernels, as build_ref.py renamed them: wmref_<kernel>_<variant> ---- */
#define KERNELS(V)                                                                                                     \
    void wmref_nvf3_##V(const clrt_image*, float*, float*);                                                            \
    void wmref_nvf5_##V(const clrt_image*, float*, float*);                                                            \
    void wmref_nvf7_##V(const clrt_image*, float*, float*);                                                            \
    void wmref_nvf9_##V(const clrt_image*, float*, float*);                                                            \
    void wmref_scaled_neighbors_p3_##V(const clrt_image*, float*, const float*, float*);                              \
    void wmref_me_##V(const clrt_image*, float*, float*, const int*, uint16_t*);
KERNELS(mad)
KERNELS(strict)

typedef void (*nvf_fn)(const clrt_image*, float*, float*);
typedef void (*sn_fn)(const clrt_image*, float*, const float*, float*);
typedef void (*me_fn)(const clrt_image*, float*, float*, const int*, uint16_t*);

static const nvf_fn nvf_kernels[2][4] = {{wmref_nvf3_mad, wmref_nvf5_mad, wmref_nvf7_mad, wmref_nvf9_mad},
                                         {wmref_nvf3_strict, wmref_nvf5_strict, wmref_nvf7_strict, wmref_nvf9_strict}};
static const sn_fn sn_kernels[2] = {wmref_scaled_neighbors_p3_mad, wmref_scaled_neighbors_p3_strict};
static const me_fn me_kernels[2] = {wmref_me_mad, wmref_me_strict};

/* the reference's RxMappings[64] (Watermark.hpp:29-39), extracted into oracle/_ref/src by build_ref.py */
static const int rx_mappings[64] =
#include "rx_mappings.inc"
    ;

/* column-major [cols][rows] (ArrayFire's layout, the kernels' store x * height + y) -> row-major [rows][cols] */
static void from_column_major(const float* cm, int rows, int cols, float* out)
{
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) out[(size_t)r * cols + c] = cm[(size_t)c * rows + r];
}

typedef struct { const clrt_image* im; float* out; nvf_fn k; } nvf_args;
static void nvf_body(void* a, void* local)
{
    const nvf_args* A = (const nvf_args*)a;
    A->k(A->im, A->out, (float*)local);
}

/* computeCustomMask (Watermark.cpp:105-121): NDRange (ALIGN16(rows), ALIGN16(cols)), local 16 x 16,
 * (16 + p)^2 floats of local memory */
int wmref_nvf(int variant, int p, const float* x, int rows, int cols, float* out)
{
    if (variant < 0 || variant > 1 || (p != 3 && p != 5 && p != 7 && p != 9) || rows < 1 || cols < 1) return -1;
    float* cm = (float*)malloc((size_t)rows * cols * sizeof(float));
    if (!cm) return -1;
    const clrt_image im = {x, rows, cols};
    nvf_args a = {&im, cm, nvf_kernels[variant][(p - 3) / 2]};
    const int st = launch(ALIGN_UP(rows, 16), ALIGN_UP(cols, 16), 16, 16, sizeof(float) * (16 + p) * (16 + p), nvf_body, &a);
    if (st == 0) from_column_major(cm, rows, cols, out);
    free(cm);
    return st;
}

typedef struct { const clrt_image* im; float* out; const float* c; sn_fn k; } sn_args;
static void sn_body(void* a, void* local)
{
    const sn_args* A = (const sn_args*)a;
    A->k(A->im, A->out, A->c, (float*)local);
}

/* computeScaledNeighbors (Watermark.cpp:124-140): NDRange (ALIGN16(rows), ALIGN16(cols)), local 16 x 16, 324 floats */
int wmref_scaled_neighbors(int variant, const float* x, int rows, int cols, const float c[8], float* out)
{
    if (variant < 0 || variant > 1 || rows < 1 || cols < 1) return -1;
    float* cm = (float*)malloc((size_t)rows * cols * sizeof(float));
    if (!cm) return -1;
    const clrt_image im = {x, rows, cols};
    sn_args a = {&im, cm, c, sn_kernels[variant]};
    const int st = launch(ALIGN_UP(rows, 16), ALIGN_UP(cols, 16), 16, 16, sizeof(float) * 324, sn_body, &a);
    if (st == 0) from_column_major(cm, rows, cols, out);
    free(cm);
    return st;
}

typedef struct { const clrt_image* im; float* Rp; float* rp; me_fn k; } me_args;
static void me_body(void* a, void* local)
{
    const me_args* A = (const me_args*)a;
    A->k(A->im, A->Rp, A->rp, rx_mappings, (uint16_t*)local);
}

/* computePredictionErrorMask's launch (Watermark.cpp:176-196): NDRange (ALIGN64(cols), rows), local 64 x 1,
 * 2304 halves.  Rp: rows x ALIGN64(cols) floats, rp: rows x ALIGN64(cols) / 8, both exactly as the kernel writes them. */
int wmref_me_partials(int variant, const float* x, int rows, int cols, float* Rp, float* rp)
{
    if (variant < 0 || variant > 1 || rows < 1 || cols < 1) return -1;
    const clrt_image im = {x, rows, cols};
    me_args a = {&im, Rp, rp, me_kernels[variant]};
    return launch(ALIGN_UP(cols, 64), (size_t)rows, 64, 1, sizeof(uint16_t) * 2304, me_body, &a);
}
