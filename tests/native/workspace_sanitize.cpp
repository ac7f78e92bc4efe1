// Host-only sanitizer harness (hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined; tests/test_sanitize.py) for the lazy
// workspaces of a context: pp_ctx_workspace and pp_ctx_free_workspaces of csrc/pp_internal.h, compiled here against stand-ins for
// hipMalloc / hipFree that take their memory from the sanitized heap, count, and fail on request.  A leak, a double free, a buffer
// shorter than the bytes asked for or a stale pointer after a failure is the sanitizer's to find.  Exit code 0 and an empty report =
// pass.  The program opens no device and is never run on one.
#include "../../packppi_amd/csrc/pp_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int g_allocs = 0, g_frees = 0;
static bool g_fail_alloc = false;
static std::string g_error;

extern "C" hipError_t hipMalloc(void **p, size_t n) {
    if (g_fail_alloc) return hipErrorOutOfMemory;
    *p = std::malloc(n);
    g_allocs++;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *p) {
    std::free(p);
    g_frees++;
    return hipSuccess;
}
extern "C" const char *hipGetErrorString(hipError_t) { return "stand-in error"; }
void pp_set_error(const std::string &msg) { g_error = msg; }

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    pp_ctx *a = new pp_ctx(), *b = new pp_ctx();
    void *first[PP_WS_COUNT], *p = nullptr;
    // the first call allocates, the second finds the allocation again; every byte asked for is there
    for (int w = 0; w < PP_WS_COUNT; w++) {
        const size_t bytes = 1000 + 24 * (size_t)w;
        EXPECT(pp_ctx_workspace(a, w, bytes, &first[w]) == PP_OK && first[w]);
        std::memset(first[w], w, bytes);
        EXPECT(pp_ctx_workspace(a, w, bytes, &p) == PP_OK && p == first[w]);
    }
    EXPECT(g_allocs == PP_WS_COUNT && g_frees == 0);
    for (int w = 0; w < PP_WS_COUNT; w++)
        for (int v = 0; v < w; v++) EXPECT(first[w] != first[v]);
    // a second context of another size has its own
    for (int w = 0; w < PP_WS_COUNT; w++) {
        EXPECT(pp_ctx_workspace(b, w, 64, &p) == PP_OK && p && p != first[w]);
        std::memset(p, 0, 64);
    }
    EXPECT(g_allocs == 2 * PP_WS_COUNT && g_frees == 0);
    // another size on the same context: the old allocation is freed, not trusted
    EXPECT(pp_ctx_workspace(a, PP_WS_POLAR, 5000, &p) == PP_OK && p);
    std::memset(p, 1, 5000);
    EXPECT(g_allocs == 2 * PP_WS_COUNT + 1 && g_frees == 1 && a->ws[PP_WS_POLAR].bytes == 5000);
    // a failed allocation behind a free leaves no pointer to the freed memory, and the next call recovers
    g_fail_alloc = true;
    EXPECT(pp_ctx_workspace(a, PP_WS_POLAR, 6000, &p) == PP_ERR_HIP && !g_error.empty());
    EXPECT(a->ws[PP_WS_POLAR].p == nullptr && a->ws[PP_WS_POLAR].bytes == 0 && g_frees == 2);
    g_fail_alloc = false;
    EXPECT(pp_ctx_workspace(a, PP_WS_POLAR, 6000, &p) == PP_OK && p);
    std::memset(p, 2, 6000);
    // destruction frees every allocation once; a context that never ran an entry frees nothing
    pp_ctx *idle = new pp_ctx();
    const int frees = g_frees;
    pp_ctx_free_workspaces(idle);
    EXPECT(g_frees == frees);
    pp_ctx_free_workspaces(a);
    pp_ctx_free_workspaces(b);
    pp_ctx_free_workspaces(b);
    EXPECT(g_allocs == g_frees);
    delete idle;
    delete a;
    delete b;
    std::printf("ok: %d allocations, %d frees\n", g_allocs, g_frees);
    return 0;
}
