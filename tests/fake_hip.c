/* tests/fake_hip.c — TEST INFRASTRUCTURE: a HIP runtime on host memory whose streams DEFER their work, for the two host pipelines
 * (lizard_amd/csrc/lizard_pipeline_host.c, lizard_unframe_host.c) on a CPU.  tests/combiner_fake.c executes every call at once and
 * so cannot see an ordering bug; here a stream is a FIFO of ops — copy, "kernel" (a host closure), event record, event wait — and
 * an op reads its arguments WHEN IT RUNS: host code that rewrites pinned staging before the copy that reads it has run, or reads a
 * result before the copy that brings it has run, gets wrong bytes, as on hardware.
 *
 * Events: hipEventRecord gives the event a new ticket (stream, sequence number of the record op); hipStreamWaitEvent captures the
 * ticket current at the call (none: a no-op, as in HIP); hipEventSynchronize / hipEventQuery refer to the latest ticket.
 * Schedules (fh_set_schedule): FH_EAGER runs every op at enqueue; FH_LAZY runs nothing until a host-side wait needs it, and then
 * only the stream up to the awaited op plus what its waits need transitively; FH_RANDOM runs a random number of ready ops of random
 * streams at every runtime call.  hipFree, hipHostFree and hipDeviceSynchronize complete everything.
 * Checks (a message, then abort — or count, see fh_set_abort): fresh allocations are filled with a poison pattern; the device side
 * of every op must lie inside a live fake device allocation, the host side of an async copy inside live fake-pinned or registered
 * memory; in an AddressSanitizer build device allocations are poisoned except while an op executes, so host code that
 * dereferences a device pointer faults.  One lock (recursive: closures may call fh_check_dev); usable under ThreadSanitizer. */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fake_hip.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define FH_POISON(p, n)   ASAN_POISON_MEMORY_REGION(p, n)
#define FH_UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define FH_POISON(p, n)   ((void)(p), (void)(n))
#define FH_UNPOISON(p, n) ((void)(p), (void)(n))
#endif

enum { OP_COPY, OP_KERNEL, OP_RECORD, OP_WAIT };
enum { MEM_DEV = 1, MEM_PINNED = 2, MEM_REGISTERED = 3 };
typedef struct FhStream FhStream;
typedef struct { FhStream* st; uint64_t seq; } Ticket;                    /* complete when st->done >= seq; st == NULL: no ticket */
typedef struct { int kind; void* dst; const void* src; size_t n; hipMemcpyKind dir; void (*fn)(void*); void* arg; Ticket wait; } Op;
struct FhStream { Op* q; size_t cap, head, tail; uint64_t done; FhStream* next; };
typedef struct { Ticket t; } FhEvent;
typedef struct { uint8_t* base; size_t size; int kind; } Mem;

static pthread_mutex_t g_mu;
static pthread_once_t g_once = PTHREAD_ONCE_INIT;
static FhStream g_null, *g_streams = &g_null;                              /* streams are never unlinked: tickets may outlive them */
static Mem g_mem[4096]; static int g_nMem;
static int g_mode = FH_EAGER, g_abort = 1, g_pageable = 0, g_violations;
static unsigned g_rng = 1u;
static char g_first[512];
static unsigned long long g_opsRun;
static int g_failMalloc;                                                   /* fh_fail_malloc: the n-th hipMalloc from now fails */

static void init_once(void)
{
    pthread_mutexattr_t a;
    pthread_mutexattr_init(&a); pthread_mutexattr_settype(&a, PTHREAD_MUTEX_RECURSIVE);
    pthread_mutex_init(&g_mu, &a);
}
static void lock(void) { pthread_once(&g_once, init_once); pthread_mutex_lock(&g_mu); }
static void unlock(void) { pthread_mutex_unlock(&g_mu); }
static unsigned rnd(void) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

static void fail(const char* fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
    fprintf(stderr, "fake_hip: %s (schedule %d, rng %u)\n", msg, g_mode, g_rng);
    if (!g_violations++) snprintf(g_first, sizeof g_first, "%s", msg);
    if (g_abort) abort();
}

static const Mem* find(const void* p, size_t n)
{
    int i;
    for (i = 0; i < g_nMem; i++)
        if (g_mem[i].kind && (const uint8_t*)p >= g_mem[i].base && (const uint8_t*)p + n <= g_mem[i].base + g_mem[i].size && n <= g_mem[i].size) return &g_mem[i];
    return NULL;
}
static void add_mem(void* p, size_t n, int kind)
{
    int i;
    for (i = 0; i < g_nMem && g_mem[i].kind; i++) {}
    if (i == 4096) { fail("allocation table full"); return; }
    if (i == g_nMem) g_nMem++;
    g_mem[i].base = (uint8_t*)p; g_mem[i].size = n; g_mem[i].kind = kind;
}
static int drop_mem(const void* p, int kindLo, int kindHi)
{
    int i;
    for (i = 0; i < g_nMem; i++)
        if (g_mem[i].kind >= kindLo && g_mem[i].kind <= kindHi && g_mem[i].base == (const uint8_t*)p) { g_mem[i].kind = 0; return 1; }
    return 0;
}
static void device_visible(int on)
{
    int i;
    for (i = 0; i < g_nMem; i++)
        if (g_mem[i].kind == MEM_DEV) { if (on) FH_UNPOISON(g_mem[i].base, g_mem[i].size); else FH_POISON(g_mem[i].base, g_mem[i].size); }
}
static int dev_ok(const void* p, size_t n, const char* what)
{
    const Mem* m = find(p, n);
    if (m) return 1;
    fail("%s: device range %p + %zu is not inside a live device allocation", what, p, n);
    return 0;
}
static int host_ok(const void* p, size_t n, const char* what)
{
    const Mem* m = find(p, n);
    if (m && m->kind != MEM_DEV) return 1;
    if (m) { fail("%s: host side %p + %zu is device memory", what, p, n); return 0; }
    if (g_pageable) return 1;
    fail("%s: host side %p + %zu of an async copy is neither fake-pinned nor registered memory", what, p, n);
    return 0;
}
static int copy_ok(const Op* o, const char* when)
{
    char what[64];
    const Mem *md = find(o->dst, o->n), *ms = find(o->src, o->n);
    hipMemcpyKind dir = o->dir;
    snprintf(what, sizeof what, "copy of %zu bytes (%s)", o->n, when);
    if (dir == hipMemcpyDefault)
        dir = (md && md->kind == MEM_DEV) ? ((ms && ms->kind == MEM_DEV) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) : hipMemcpyDeviceToHost;
    if (dir == hipMemcpyHostToDevice) return dev_ok(o->dst, o->n, what) && host_ok(o->src, o->n, what);
    if (dir == hipMemcpyDeviceToHost) return dev_ok(o->src, o->n, what) && host_ok(o->dst, o->n, what);
    if (dir == hipMemcpyDeviceToDevice) return dev_ok(o->dst, o->n, what) && dev_ok(o->src, o->n, what);
    return host_ok(o->dst, o->n, what) && host_ok(o->src, o->n, what);
}

static int ticket_done(Ticket t) { return !t.st || t.st->done >= t.seq; }
static uint64_t enqueued(const FhStream* s) { return s->done + (s->tail - s->head); }

static void run_head(FhStream* s)                                /* the head op is ready */
{
    Op o = s->q[s->head];
    if (o.kind == OP_COPY) {
        if (o.n && copy_ok(&o, "at execution")) { device_visible(1); memmove(o.dst, o.src, o.n); device_visible(0); }
    } else if (o.kind == OP_KERNEL) {
        device_visible(1); o.fn(o.arg); device_visible(0);
        free(o.arg);
    }
    s->head++; s->done++;
    if (s->head == s->tail) s->head = s->tail = 0;
    g_opsRun++;
}
static void run_until(FhStream* s, uint64_t seq)
{
    while (s->done < seq && s->head < s->tail) {
        const Op* o = &s->q[s->head];
        if (o->kind == OP_WAIT && !ticket_done(o->wait)) run_until(o->wait.st, o->wait.seq);     /* recorded before the wait was enqueued: no cycles */
        run_head(s);
    }
}
static void run_all(void) { FhStream* s; for (s = g_streams; s; s = s->next) run_until(s, enqueued(s)); }
static void pump(void)                                           /* FH_RANDOM: a few ready ops of random streams */
{
    unsigned k;
    if (g_mode != FH_RANDOM) return;
    for (k = rnd() % 5u; k; k--) {
        FhStream *s, *pick = NULL; unsigned seen = 0;
        for (s = g_streams; s; s = s->next) {
            if (s->head == s->tail) continue;
            if (s->q[s->head].kind == OP_WAIT && !ticket_done(s->q[s->head].wait)) continue;
            if (rnd() % ++seen == 0) pick = s;
        }
        if (!pick) return;
        run_head(pick);
    }
}
static FhStream* stream_of(hipStream_t st) { return st ? (FhStream*)st : &g_null; }
static uint64_t enqueue(FhStream* s, const Op* o)
{
    uint64_t seq;
    if (s->tail == s->cap) {
        s->cap = s->cap ? 2 * s->cap : 64;
        s->q = (Op*)realloc(s->q, s->cap * sizeof(Op));
        if (!s->q) abort();
    }
    s->q[s->tail++] = *o;
    seq = enqueued(s);
    if (g_mode == FH_EAGER) run_until(s, seq);
    return seq;
}

/* ---- controls ---- */
void fh_set_schedule(int mode, unsigned seed) { lock(); run_all(); g_mode = mode; g_rng = seed ? seed : 1u; unlock(); }
void fh_set_abort(int on) { lock(); g_abort = on; unlock(); }
int  fh_violations(char* first, size_t cap)
{
    int n;
    lock();
    n = g_violations;
    if (first && cap) snprintf(first, cap, "%s", n ? g_first : "");
    g_violations = 0; g_first[0] = 0;
    unlock();
    return n;
}
void fh_register_pinned(const void* p, size_t n) { lock(); add_mem((void*)(uintptr_t)p, n, MEM_REGISTERED); unlock(); }
void fh_unregister_pinned(const void* p) { lock(); run_all(); if (!drop_mem(p, MEM_REGISTERED, MEM_REGISTERED)) fail("fh_unregister_pinned(%p): not registered", p); unlock(); }
void fh_allow_pageable(int on) { lock(); g_pageable += on ? 1 : (g_pageable > 0 ? -1 : 0); unlock(); }      /* (a count: several threads may ask) */
int  fh_check_dev(const void* p, size_t n, const char* what) { int ok; lock(); ok = dev_ok(p, n, what); unlock(); return ok; }
void fh_fail_malloc(int nth) { lock(); g_failMalloc = nth; unlock(); }
unsigned fh_rand(void) { unsigned r; lock(); r = rnd(); unlock(); return r; }
unsigned long long fh_ops_run(void) { unsigned long long v; lock(); v = g_opsRun; unlock(); return v; }
void fh_assert_idle(const char* where)
{
    FhStream* s; size_t left = 0;
    lock();
    for (s = g_streams; s; s = s->next) left += s->tail - s->head;
    if (left) { fail("%s: %zu ops are still queued", where, left); run_all(); }
    unlock();
}
hipError_t fh_enqueue_kernel(hipStream_t st, void (*fn)(void*), const void* arg, size_t argBytes)
{
    Op o;
    memset(&o, 0, sizeof o);
    o.kind = OP_KERNEL; o.fn = fn; o.arg = malloc(argBytes ? argBytes : 1);
    if (!o.arg) return hipErrorOutOfMemory;
    memcpy(o.arg, arg, argBytes);
    lock(); pump(); enqueue(stream_of(st), &o); unlock();
    return hipSuccess;
}

/* ---- the runtime ---- */
static hipError_t alloc_mem(void** p, size_t n, int kind, int fill)
{
    void* q = malloc(n ? n : 1);
    if (!q) { *p = NULL; return hipErrorOutOfMemory; }
    memset(q, fill, n ? n : 1);
    lock(); pump(); add_mem(q, n ? n : 1, kind); if (kind == MEM_DEV) FH_POISON(q, n ? n : 1); unlock();
    *p = q;
    return hipSuccess;
}
static hipError_t free_mem(void* p, int kind, const char* name)
{
    const Mem* m;
    size_t size;
    if (!p) return hipSuccess;
    lock();
    run_all();
    m = find(p, 1);
    if (!m || m->base != (uint8_t*)p || m->kind != kind) { fail("%s(%p): not a live allocation of that kind", name, p); unlock(); return hipErrorInvalidValue; }
    size = m->size;
    drop_mem(p, kind, kind);
    unlock();
    FH_UNPOISON(p, size);                                    /* (free() of a region poisoned by hand is reported otherwise) */
    free(p);
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n)
{
    int refuse;
    lock(); refuse = g_failMalloc && !--g_failMalloc; unlock();
    if (refuse) { *p = NULL; return hipErrorOutOfMemory; }
    return alloc_mem(p, n, MEM_DEV, 0xD5);
}
hipError_t hipFree(void* p) { return free_mem(p, MEM_DEV, "hipFree"); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned flags) { (void)flags; return alloc_mem(p, n, MEM_PINNED, 0xB6); }
hipError_t hipHostFree(void* p) { return free_mem(p, MEM_PINNED, "hipHostFree"); }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    Op o;
    memset(&o, 0, sizeof o);
    o.kind = OP_COPY; o.dst = d; o.src = s; o.n = n; o.dir = k;
    lock(); pump();
    if (!n || copy_ok(&o, "at enqueue")) enqueue(stream_of(st), &o);
    unlock();
    return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k)
{
    (void)k;
    lock(); run_until(&g_null, enqueued(&g_null)); device_visible(1); memmove(d, s, n); device_visible(0); unlock();
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* st, unsigned f)
{
    FhStream* s = (FhStream*)calloc(1, sizeof *s);
    (void)f;
    if (!s) return hipErrorOutOfMemory;
    lock(); s->next = g_streams; g_streams = s; unlock();
    *st = (hipStream_t)s;
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t st) { FhStream* s = stream_of(st); lock(); run_until(s, enqueued(s)); unlock(); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t st) { FhStream* s = stream_of(st); lock(); pump(); run_until(s, enqueued(s)); unlock(); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { lock(); run_all(); unlock(); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { *e = (hipEvent_t)calloc(1, sizeof(FhEvent)); return *e ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned f) { (void)f; return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t e) { lock(); run_all(); unlock(); free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st)
{
    FhEvent* ev = (FhEvent*)e; FhStream* s = stream_of(st);
    Op o;
    if (!ev) return hipErrorInvalidHandle;
    memset(&o, 0, sizeof o);
    o.kind = OP_RECORD;
    lock(); pump();
    ev->t.st = s; ev->t.seq = enqueued(s) + 1;                /* the ticket first: an eager enqueue completes it at once */
    enqueue(s, &o);
    unlock();
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t e, unsigned f)
{
    FhEvent* ev = (FhEvent*)e;
    Op o;
    (void)f;
    if (!ev) return hipErrorInvalidHandle;
    memset(&o, 0, sizeof o);
    o.kind = OP_WAIT;
    lock(); pump();
    o.wait = ev->t;
    if (o.wait.st) enqueue(stream_of(st), &o);                /* never recorded: a no-op */
    unlock();
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    FhEvent* ev = (FhEvent*)e;
    if (!ev) return hipErrorInvalidHandle;
    lock(); pump(); if (ev->t.st) run_until(ev->t.st, ev->t.seq); unlock();
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e)
{
    FhEvent* ev = (FhEvent*)e; int done;
    if (!ev) return hipErrorInvalidHandle;
    lock(); pump(); done = ticket_done(ev->t); unlock();
    return done ? hipSuccess : hipErrorNotReady;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b)
{
    FhEvent *x = (FhEvent*)a, *y = (FhEvent*)b; hipError_t r = hipSuccess;
    *ms = 0.0f;
    if (!x || !y) return hipErrorInvalidHandle;
    lock();
    if (!x->t.st || !y->t.st) r = hipErrorInvalidHandle;
    else if (!ticket_done(x->t) || !ticket_done(y->t)) r = hipErrorNotReady;
    unlock();
    return r;
}
hipError_t hipSetDevice(int d) { (void)d; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t e) { (void)e; return "fake"; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned f) { (void)f; *d = h; return hipSuccess; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* p)
{
    const Mem* m;
    memset(a, 0, sizeof *a);
    lock(); m = find(p, 1);
    if (m) a->type = m->kind == MEM_DEV ? hipMemoryTypeDevice : hipMemoryTypeHost;
    unlock();
    return m ? hipSuccess : hipErrorInvalidValue;
}
