/* tests/fake_hip.h — TEST INFRASTRUCTURE: controls of the fake HIP runtime with deferred streams (tests/fake_hip.c). */
#ifndef FAKE_HIP_H
#define FAKE_HIP_H
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
enum { FH_EAGER = 0, FH_LAZY = 1, FH_RANDOM = 2 };
void fh_set_schedule(int mode, unsigned seed);
/* 1 (default): a failed check prints its message and aborts.  0: it is printed, counted and kept for fh_violations, and the
 * offending op is not executed (an in-process caller, such as a ctypes test, asserts on the count after every call). */
void fh_set_abort(int on);
int  fh_violations(char* firstMessage, size_t cap);          /* count since the last call; resets */
/* caller memory the test declares pinned (hipHostRegister's effect): hipPointerGetAttributes answers "host" for it and async
 * copies may use it */
void fh_register_pinned(const void* p, size_t n);
void fh_unregister_pinned(const void* p);
/* 1: an async copy whose host side is pageable memory is accepted and deferred like any other (the loosest behaviour the API
 * allows; for entries that pass caller memory to hipMemcpyAsync on purpose and synchronise before they return).  0 (default): a check failure. */
void fh_allow_pageable(int on);
/* a "kernel": fn(copy of arg) runs when the stream reaches it */
hipError_t fh_enqueue_kernel(hipStream_t st, void (*fn)(void*), const void* arg, size_t argBytes);
/* [p, p + n) lies inside one live fake device allocation (or fake-pinned / registered memory, which the device can address too);
 * a failure is reported under `what` and 0 is returned */
int  fh_check_dev(const void* p, size_t n, const char* what);
void fh_assert_idle(const char* where);                       /* every stream's queue is empty, or a check failure */
unsigned fh_rand(void);
void fh_fail_malloc(int nth);                                  /* the nth hipMalloc from now answers hipErrorOutOfMemory, once (0: none) */
unsigned long long fh_ops_run(void);
#ifdef __cplusplus
}
#endif
#endif
