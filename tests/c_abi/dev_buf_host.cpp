// rscm::DevBuf and rscm::dev_malloc (rscm_amd/csrc/dev_buf.hpp) on the host, against counting stubs of the four HIP calls the header
// makes: no HIP library is linked and no device is touched.  Built with -fsanitize=address,undefined by tests/test_host_dev_buf.py,
// which runs it once plainly and once with RSCM_POISON_ALLOC=1.  Every scenario ends with no live allocation; exit status 0 and
// "dev_buf ok" on stdout if all hold, else the failed checks on stderr and exit status 1.
#include "dev_buf.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
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

// a handle in small: several owners and an array of four, as rscm_ens has d_* members and d_ind[4]
struct Handle {
    DevBuf<double> a, b;
    DevBuf<int32_t> c;
    DevBuf<unsigned char> d;
    DevBuf<double> slots[4];
};

// "build aside, move in": the member's new contents are allocated in a local; `leave` is a failure before the move
hipError_t replace_table(Handle& h, size_t n, bool leave)
{
    DevBuf<double> d_new;
    CHK(d_new.alloc(n));
    if (leave) return hipErrorInvalidValue;
    h.a = std::move(d_new);
    return hipSuccess;
}

// create_handle in small: the object lives in a unique_ptr until everything that can fail has succeeded
hipError_t create(Handle** out)
{
    std::unique_ptr<Handle> h(new Handle());
    CHK(h->a.alloc(8));
    CHK(h->c.alloc(8));
    CHK(h->slots[2].alloc(8));
    *out = h.release();
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
        CHECK(c.get() == pa && c.size() == 4 && g_frees == 1);
    }
    CHECK(g_live == 0 && g_mallocs == 2 && g_frees == 2);

    // size() follows alloc, a move and a failed alloc; an empty owner reads as a null pointer
    reset_counts();
    {
        DevBuf<double> a;
        CHECK(a.size() == 0 && a == nullptr);
        CHECK(a.alloc(7) == hipSuccess && a.size() == 7);
        double* p = a;   // the implicit conversion every reader of a handle member goes through
        CHECK(p == a.get() && a + 1 == p + 1);
        DevBuf<double> b(std::move(a));
        CHECK(a.size() == 0 && b.size() == 7);
        g_fail_at = 1;
        CHECK(b.alloc(9) == hipErrorOutOfMemory);
        CHECK(!b && b.size() == 0 && g_frees == 1 && g_last_freed == p && g_live == 0);
    }
    CHECK(g_live == 0 && g_frees == 1);

    // reserve(): smaller than, equal to and larger than size() -- no call, no call, one free and one allocation
    reset_counts();
    {
        DevBuf<int64_t> a;
        CHECK(a.reserve(0) == hipSuccess && !a && g_mallocs == 0);   // nothing asked of an empty owner
        CHECK(a.reserve(8) == hipSuccess && a.size() == 8 && g_mallocs == 1 && g_frees == 0);
        int64_t* first = a.get();
        CHECK(a.reserve(4) == hipSuccess && a.get() == first && a.size() == 8);
        CHECK(a.reserve(8) == hipSuccess && a.get() == first && a.size() == 8);
        CHECK(g_mallocs == 1 && g_frees == 0);
        CHECK(a.reserve(9) == hipSuccess && a.size() == 9);
        a.get()[8] = 1;   // the whole of it is there
        CHECK(g_mallocs == 2 && g_frees == 1 && g_last_freed == first && g_live == 1);
    }
    CHECK(g_live == 0 && g_frees == 2);

    // reserve() whose allocation fails: empty, size() == 0, the old block freed exactly once (and not again by the destructor)
    reset_counts();
    {
        DevBuf<double> a;
        CHECK(a.alloc(4) == hipSuccess);
        double* first = a.get();
        g_fail_at = 1;
        CHECK(a.reserve(16) == hipErrorOutOfMemory);
        CHECK(!a && a.get() == nullptr && a.size() == 0 && g_frees == 1 && g_last_freed == first && g_live == 0);
        CHECK(a.reserve(2) == hipSuccess && a.size() == 2);   // and the owner is usable afterwards
    }
    CHECK(g_live == 0 && g_mallocs == 3 && g_frees == 2);

    // reset(): frees, leaves the owner empty, and is harmless on an empty one
    reset_counts();
    {
        DevBuf<double> a;
        a.reset();
        CHECK(g_frees == 0);
        CHECK(a.alloc(4) == hipSuccess);
        a.reset();
        CHECK(!a && a.size() == 0 && g_frees == 1 && g_live == 0);
        a.reset();
        CHECK(g_frees == 1);
    }
    CHECK(g_live == 0 && g_frees == 1);

    // move-assignment of a local into a member: the member's old block is freed once, the local ends empty and
    // no longer frees the new one; into an empty member there is nothing to free
    reset_counts();
    {
        Handle h;
        CHECK(h.c.alloc(4) == hipSuccess);
        int32_t* old = h.c.get();
        {
            DevBuf<int32_t> d_new;
            CHECK(d_new.alloc(6) == hipSuccess);
            int32_t* fresh = d_new.get();
            h.c = std::move(d_new);
            CHECK(!d_new && d_new.size() == 0 && h.c.get() == fresh && h.c.size() == 6 && g_frees == 1 && g_last_freed == old);
        }
        CHECK(g_live == 1 && g_frees == 1);
        {
            DevBuf<double> d_new;
            CHECK(d_new.alloc(4) == hipSuccess);
            h.b = std::move(d_new);
            CHECK(g_frees == 1 && h.b && h.b.size() == 4);
        }
        CHECK(g_live == 2);
        h.c = DevBuf<int32_t>();   // an empty owner moved in: the member's block goes
        CHECK(!h.c && g_frees == 2 && g_live == 1);
    }
    CHECK(g_live == 0 && g_mallocs == 3 && g_frees == 3);

    // a struct of owners and an array of four, some empty and some full: the destructor frees every block once
    reset_counts();
    {
        Handle h;
        CHECK(h.a.alloc(3) == hipSuccess && h.d.alloc(5) == hipSuccess);
        CHECK(h.slots[1].reserve(2) == hipSuccess && h.slots[3].reserve(2) == hipSuccess);
        CHECK(g_live == 4 && !h.b && !h.c && !h.slots[0] && !h.slots[2]);
        CHECK(g_fills == (poison ? 4 : 0));
    }
    CHECK(g_live == 0 && g_mallocs == 4 && g_frees == 4);

    // build aside, fail before the move: the member still holds its old block and its old size()
    reset_counts();
    {
        Handle h;
        CHECK(replace_table(h, 4, false) == hipSuccess);
        double* old = h.a.get();
        CHECK(replace_table(h, 8, true) == hipErrorInvalidValue);
        CHECK(h.a.get() == old && h.a.size() == 4 && g_live == 1 && g_mallocs == 2 && g_frees == 1 && g_last_freed != old);
        g_fail_at = 1;   // ... and so when the allocation aside is what fails
        CHECK(replace_table(h, 8, false) == hipErrorOutOfMemory);
        CHECK(h.a.get() == old && h.a.size() == 4 && g_live == 1 && g_frees == 1);
        CHECK(replace_table(h, 8, false) == hipSuccess);
        CHECK(h.a.size() == 8 && g_last_freed == old && g_live == 1);
    }
    CHECK(g_live == 0);

    // a half-built object in a unique_ptr whose third allocation fails: nothing stays live, nothing is handed out
    reset_counts();
    {
        Handle* made = nullptr;
        g_fail_at = 3;
        CHECK(create(&made) == hipErrorOutOfMemory);
        CHECK(made == nullptr && g_live == 0 && g_mallocs == 3 && g_frees == 2);
        CHECK(create(&made) == hipSuccess && made != nullptr && g_live == 3);
        delete made;   // the whole teardown
    }
    CHECK(g_live == 0 && g_frees == 5);

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
