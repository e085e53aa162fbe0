// rscm::DevBuf and rscm::dev_malloc (rscm_amd/csrc/dev_buf.hpp) on the host, against counting stubs of the four HIP calls the header
// makes: no HIP library is linked and no device is touched.  Built with -fsanitize=address,undefined by tests/test_host_dev_buf.py,
// which runs it once plainly and once with RSCM_POISON_ALLOC=1.  Every scenario ends with no live allocation; exit status 0 and
// "dev_buf ok" on stdout if all hold, else the failed checks on stderr and exit status 1.
#include "dev_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <utility>

namespace {

long g_live = 0, g_mallocs = 0, g_frees = 0, g_fills = 0, g_syncs = 0;
long g_fail_at = 0;       // > 0: the g_fail_at-th hipMalloc from now fails with hipErrorOutOfMemory
void* g_last_freed = nullptr;
int g_failed = 0;

void reset_counts() { g_mallocs = g_frees = g_fills = g_syncs = 0; g_fail_at = 0; g_last_freed = nullptr; }

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                          \
        }                                                                        \
    } while (0)

// what HIPCHK does in the library: return past whatever is live
#define CHK(expr)                          \
    do {                                   \
        const hipError_t e_ = (expr);      \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

}  // namespace

extern "C" {

hipError_t hipMalloc(void** ptr, size_t size)
{
    ++g_mallocs;
    if (g_fail_at > 0 && --g_fail_at == 0) return hipErrorOutOfMemory;
    if (size == 0) {
        *ptr = nullptr;
        return hipSuccess;
    }
    *ptr = std::malloc(size);
    if (!*ptr) return hipErrorOutOfMemory;
    ++g_live;
    return hipSuccess;
}

hipError_t hipFree(void* ptr)
{
    if (!ptr) return hipSuccess;
    ++g_frees;
    --g_live;
    g_last_freed = ptr;
    std::free(ptr);
    return hipSuccess;
}

hipError_t hipMemset(void* dst, int value, size_t n)
{
    ++g_fills;
    std::memset(dst, value, n);
    return hipSuccess;
}

hipError_t hipDeviceSynchronize(void)
{
    ++g_syncs;
    return hipSuccess;
}

}  // extern "C"

namespace {

using rscm::DevBuf;

hipError_t early_return(bool leave)
{
    DevBuf<double> a, b;
    CHK(a.alloc(16));
    a.get()[15] = 1.0;   // the whole of it is there
    if (leave) return hipErrorInvalidValue;   // a validation failure between two allocations
    CHK(b.alloc(16));
    return hipSuccess;
}

hipError_t three_allocations()
{
    DevBuf<double> a;
    DevBuf<int32_t> b;
    DevBuf<unsigned char> c;
    CHK(a.alloc(8));
    CHK(b.alloc(8));
    CHK(c.alloc(8));
    return hipSuccess;
}

void thrower()
{
    DevBuf<double> a;
    if (a.alloc(32) != hipSuccess) return;
    throw std::runtime_error("past a live owner");
}

void scenarios(bool poison)
{
    // normal scope exit
    reset_counts();
    {
        DevBuf<double> a;
        CHECK(!a && a.get() == nullptr);
        CHECK(a.alloc(100) == hipSuccess);
        CHECK(a && g_live == 1);
        if (poison) {
            unsigned char ff[sizeof(double)];
            std::memset(ff, 0xFF, sizeof ff);
            CHECK(std::memcmp(a.get() + 99, ff, sizeof ff) == 0);
        }
    }
    CHECK(g_live == 0 && g_mallocs == 1 && g_frees == 1);

    // early return between two allocations
    reset_counts();
    CHECK(early_return(true) == hipErrorInvalidValue);
    CHECK(g_live == 0 && g_mallocs == 1 && g_frees == 1);
    CHECK(early_return(false) == hipSuccess);
    CHECK(g_live == 0 && g_mallocs == 3 && g_frees == 3);

    // the second of three allocations fails: the first is freed, the code comes through unchanged
    reset_counts();
    g_fail_at = 2;
    CHECK(three_allocations() == hipErrorOutOfMemory);
    CHECK(g_live == 0 && g_mallocs == 2 && g_frees == 1);

    // a second alloc on one owner replaces what it held
    reset_counts();
    {
        DevBuf<int64_t> a;
        CHECK(a.alloc(4) == hipSuccess);
        int64_t* first = a.get();
        CHECK(a.alloc(8) == hipSuccess);
        CHECK(g_frees == 1 && g_last_freed == first && g_live == 1);
    }
    CHECK(g_live == 0 && g_frees == 2);

    // move construction and move assignment: the old pointer is freed exactly once
    reset_counts();
    {
        DevBuf<double> a;
        CHECK(a.alloc(4) == hipSuccess);
        double* pa = a.get();
        DevBuf<double> b(std::move(a));
        CHECK(!a && b.get() == pa && g_frees == 0);
        DevBuf<double> c;
        CHECK(c.alloc(4) == hipSuccess);
        double* pc = c.get();
        c = std::move(b);
        CHECK(!b && c.get() == pa && g_frees == 1 && g_last_freed == pc && g_live == 1);
        DevBuf<double>& self = c;
        c = std::move(self);
        CHECK(c.get() == pa && g_frees == 1);
    }
    CHECK(g_live == 0 && g_mallocs == 2 && g_frees == 2);

    // release(): nothing is freed, the caller's free brings the count to zero
    reset_counts();
    double* raw = nullptr;
    {
        DevBuf<double> a;
        CHECK(a.alloc(4) == hipSuccess);
        raw = a.release();
        CHECK(!a && raw != nullptr);
    }
    CHECK(g_live == 1 && g_frees == 0);
    CHECK(hipFree(raw) == hipSuccess);
    CHECK(g_live == 0 && g_frees == 1);

    // install(): the slot's old pointer is freed once and the owner no longer frees the new one
    reset_counts();
    int32_t* slot = nullptr;
    CHECK(rscm::dev_malloc(&slot, 4 * sizeof(int32_t)) == hipSuccess);
    int32_t* old = slot;
    {
        DevBuf<int32_t> a;
        CHECK(a.alloc(4) == hipSuccess);
        int32_t* fresh = a.get();
        a.install(slot);
        CHECK(!a && slot == fresh && g_frees == 1 && g_last_freed == old);
    }
    CHECK(g_live == 1 && g_frees == 1);
    {
        DevBuf<int32_t> a;   // into an empty slot: nothing to free
        int32_t* empty = nullptr;
        CHECK(a.alloc(4) == hipSuccess);
        a.install(empty);
        CHECK(g_frees == 1 && empty != nullptr);
        CHECK(hipFree(empty) == hipSuccess);
    }
    CHECK(hipFree(slot) == hipSuccess);
    CHECK(g_live == 0 && g_mallocs == 3 && g_frees == 3);

    // an exception thrown past a live owner
    reset_counts();
    bool caught = false;
    try {
        thrower();
    } catch (const std::runtime_error&) {
        caught = true;
    }
    CHECK(caught && g_live == 0 && g_mallocs == 1 && g_frees == 1);

    // RSCM_POISON_ALLOC: an allocation is followed by one fill and one device sync, a zero-byte allocation by neither
    reset_counts();
    {
        DevBuf<double> a, z;
        CHECK(a.alloc(10) == hipSuccess);
        CHECK(g_fills == (poison ? 1 : 0) && g_syncs == (poison ? 1 : 0));
        CHECK(z.alloc(0) == hipSuccess);
        CHECK(g_fills == (poison ? 1 : 0) && g_syncs == (poison ? 1 : 0) && g_mallocs == 2);
        g_fail_at = 1;   // a failed allocation is not filled either
        DevBuf<double> f;
        CHECK(f.alloc(10) == hipErrorOutOfMemory && !f);
        CHECK(g_fills == (poison ? 1 : 0) && g_syncs == (poison ? 1 : 0));
    }
    CHECK(g_live == 0);
}

}  // namespace

int main()
{
    const char* e = std::getenv("RSCM_POISON_ALLOC");
    const bool poison = e && std::atoi(e) != 0;
    scenarios(poison);
    if (g_failed || g_live != 0) {
        std::fprintf(stderr, "dev_buf: %d checks failed, %ld allocations live\n", g_failed, g_live);
        return 1;
    }
    std::printf("dev_buf ok (poison %s)\n", poison ? "on" : "off");
    return 0;
}
