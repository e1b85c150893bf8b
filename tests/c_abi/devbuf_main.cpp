// DevBuf<T> (csrc/bcp_devbuf.h) on the host alone: hipMalloc / hipFree are malloc / free here, with a switch that makes
// the next allocation fail.  Built with -fsanitize=address,undefined and no HIP library: a buffer that is not freed is
// what the leak check at exit reports, a buffer freed twice or used after its free is what the sanitizer stops at.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "bcp_devbuf.h"
#include "host_io.h"

static bool g_fail_next = false;
static int g_live = 0, g_mallocs = 0, g_frees = 0;

extern "C" hipError_t hipMalloc(void** ptr, size_t size)
{
    if (g_fail_next) {
        g_fail_next = false;
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    *ptr = malloc(size ? size : 1);
    if (!*ptr) return hipErrorOutOfMemory;
    memset(*ptr, 0xA5, size);
    ++g_live;
    ++g_mallocs;
    return hipSuccess;
}

extern "C" hipError_t hipFree(void* ptr)
{
    if (ptr) {
        --g_live;
        ++g_frees;
    }
    free(ptr);
    return hipSuccess;
}


struct Wide {
    double d[5];
};

int main()
{
    {
        DevBuf<int> b;
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(0) == hipSuccess && b.get() == nullptr && g_mallocs == 0);   // nothing asked, nothing done

        // growth allocates, and the whole capacity can be written
        CHECK(b.reserve(100) == hipSuccess && b.get() != nullptr && b.capacity() == 100);
        CHECK(g_live == 1 && g_mallocs == 1);
        for (int i = 0; i < 100; ++i) b.get()[i] = i;

        // an equal or smaller request keeps pointer and capacity
        int* const first = b.get();
        CHECK(b.reserve(100) == hipSuccess && b.get() == first && b.capacity() == 100);
        CHECK(b.reserve(7) == hipSuccess && b.get() == first && b.capacity() == 100);
        CHECK(g_mallocs == 1 && g_frees == 0);
        CHECK(first[99] == 99);

        // growth frees the old block before it takes the new one: never two at once
        CHECK(b.reserve(101) == hipSuccess && b.capacity() == 101 && g_live == 1 && g_mallocs == 2 && g_frees == 1);
        b.get()[100] = 1;

        // a failed growth leaves the buffer empty -- the old block is gone, too -- and a later reserve works
        g_fail_next = true;
        CHECK(b.reserve(1000) == hipErrorOutOfMemory);
        CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 0);
        CHECK(b.reserve(5) == hipSuccess && b.get() != nullptr && b.capacity() == 5 && g_live == 1);
        b.get()[4] = 4;

        // reset frees, twice is once, and the buffer can be used again
        CHECK(b.reset() == hipSuccess && b.get() == nullptr && b.capacity() == 0 && g_live == 0);
        CHECK(b.reset() == hipSuccess && g_live == 0);
        CHECK(b.reserve(3) == hipSuccess && g_live == 1);
    }
    CHECK(g_live == 0);   // the destructor freed

    {   // the capacity counts elements, not bytes
        DevBuf<Wide> w;
        CHECK(w.reserve(9) == hipSuccess && w.capacity() == 9);
        w.get()[8].d[4] = 1.0;
        DevBuf<Wide> never_used;
    }
    CHECK(g_live == 0 && g_mallocs == g_frees);

    static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value,
                  "one owner per block");
    if (g_failed) return 1;
    printf("devbuf ok: %d allocations, %d frees\n", g_mallocs, g_frees);
    return 0;
}
