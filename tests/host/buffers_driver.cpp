// buffers_driver.cpp -- stand-alone driver of movi_amd/csrc/movi_buffers.hpp for a sanitizer build (host code only, no GPU):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o buffers_driver tests/host/buffers_driver.cpp && ./buffers_driver
// The owning types on a malloc-backed policy that counts its calls, live blocks and live bytes: reserve() within capacity calls
// nothing; a growth frees before it allocates; the four slack rules give the library's capacities; a failed allocation leaves the
// buffer empty; moves; a marked graph-safe buffer that grows keeps its old block alive and counted until release(); nothing is live
// after release() or destruction.  (A leak, a double free or a use after free is the sanitizer's report.)
#include "../../movi_amd/csrc/movi_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

using namespace movi;

#define REQUIRE(c)                                                                     \
    do {                                                                               \
        if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

struct CountingMem {
    using error = int;
    static constexpr error ok = 0;
    static inline std::map<void *, size_t> live;
    static inline size_t live_bytes = 0, allocs = 0, frees = 0, peak_blocks = 0;
    static inline bool fail_next = false;
    static error alloc(void **p, size_t bytes) {
        ++allocs;
        if (fail_next) { fail_next = false; return 2; }      // (*p is left as it was, like a failed hipMalloc)
        *p = malloc(bytes ? bytes : 1);
        memset(*p, 0xAB, bytes);                             // every byte of the stated size is the buffer's
        live[*p] = bytes;
        live_bytes += bytes;
        if (live.size() > peak_blocks) peak_blocks = live.size();
        return ok;
    }
    static void free(void *p) {
        ++frees;
        REQUIRE(live.count(p) == 1);
        live_bytes -= live[p];
        live.erase(p);
        ::free(p);
    }
    static size_t calls() { return allocs + frees; }
};
using Buf = GrowBuf<CountingMem>;
using GraphBuf = GraphSafeBuf<CountingMem>;
using Ptr = OwnedPtr<unsigned, CountingMem>;

static int g_cases = 0;

// one slack rule: from empty, `need` gives capacity `cap`; within it nothing is called; one past it frees first, then allocates
template <typename Rule>
static void slack(Rule rule, size_t need, size_t cap, size_t next_need) {
    {
        Buf b;
        const size_t c0 = CountingMem::calls();
        REQUIRE(rule(b, need) == 0);
        REQUIRE(b.cap() == cap && CountingMem::live_bytes == cap && (cap == 0 || b.ptr()));
        REQUIRE(CountingMem::calls() == c0 + (cap ? 1 : 0));
        const void *p = b.ptr();
        const size_t c1 = CountingMem::calls();
        REQUIRE(rule(b, need) == 0 && rule(b, next_need - 1) == 0 && rule(b, 0) == 0);
        REQUIRE(CountingMem::calls() == c1 && b.ptr() == p && b.cap() == cap);   // within capacity: no allocator call at all
        CountingMem::peak_blocks = CountingMem::live.size();
        const size_t f = CountingMem::frees;
        REQUIRE(rule(b, next_need) == 0);
        REQUIRE(b.cap() >= next_need && CountingMem::live_bytes == b.cap());
        REQUIRE(CountingMem::frees == f + (cap ? 1 : 0) && CountingMem::peak_blocks <= 1);   // freed BEFORE the new block came
    }
    REQUIRE(CountingMem::live.empty() && CountingMem::live_bytes == 0);
    ++g_cases;
}

int main() {
    // ---- the slack rules, with the library's numbers
    auto dev = [](Buf &b, size_t n) { return grow(b, n); };                  // >= 8 bytes, an eighth on top
    for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8}) slack(dev, n, 9, 10);
    slack(dev, 9, 10, 11);
    slack(dev, 1000, 1125, 1126);
    slack(dev, (size_t)1 << 24, ((size_t)1 << 24) + ((size_t)1 << 21), ((size_t)1 << 24) + ((size_t)1 << 21) + 1);
    auto ent = [](Buf &b, size_t n) { return grow_entries(b, n); };          // entries + entries / 8, 8 bytes each
    slack(ent, 0, 0, 1);
    slack(ent, 1, 8, 2);
    slack(ent, 8, 72, 10);
    slack(ent, 1001, (1001 + 125) * 8, 1127);
    auto blk = [](Buf &b, size_t n) { return grow_block(b, n); };            // bytes + bytes / 4
    slack(blk, 0, 0, 1);
    slack(blk, 1, 1, 2);
    slack(blk, 4, 5, 6);
    slack(blk, 1000, 1250, 1251);
    auto own = [](Buf &b, size_t n) { return b.reserve(n, n == 64 ? 4096 : n + (n >> 3)); };   // the segment workspace: the caller's own `alloc`
    slack(own, 0, 0, 1);
    slack(own, 1, 1, 2);
    slack(own, 64, 4096, 4097);
    slack(own, 100000, 112500, 112501);

    // ---- a failed allocation leaves the buffer empty -- also one that held a block
    {
        Buf b;
        CountingMem::fail_next = true;
        REQUIRE(grow(b, 100) != 0 && b.ptr() == nullptr && b.cap() == 0 && CountingMem::live.empty());
        REQUIRE(grow(b, 100) == 0 && b.cap() == 112);
        CountingMem::fail_next = true;
        REQUIRE(grow(b, 1000) != 0 && b.ptr() == nullptr && b.cap() == 0 && CountingMem::live.empty());
        REQUIRE(grow(b, 10) == 0 && b.cap() == 11);         // and it is usable afterwards
        ++g_cases;
    }
    REQUIRE(CountingMem::live.empty());

    // ---- moves: the block changes hands, the source is empty, the target's old block is freed
    {
        Buf a, b;
        REQUIRE(grow(a, 100) == 0 && grow(b, 200) == 0 && CountingMem::live.size() == 2);
        void *pa = a.ptr();
        Buf c(std::move(a));
        REQUIRE(c.ptr() == pa && c.cap() == 112 && a.ptr() == nullptr && a.cap() == 0 && CountingMem::live.size() == 2);
        b = std::move(c);
        REQUIRE(b.ptr() == pa && b.cap() == 112 && c.ptr() == nullptr && CountingMem::live.size() == 1 && CountingMem::live_bytes == 112);
        Buf &same = b;
        b = std::move(same);                                 // (self-move: nothing happens)
        REQUIRE(b.ptr() == pa && CountingMem::live.size() == 1);
        b.release();
        REQUIRE(b.ptr() == nullptr && b.cap() == 0 && CountingMem::live.empty());
        b.release();                                         // (twice: nothing happens)
        ++g_cases;
    }

    // ---- the graph-safe buffer: two buffers on one retired list
    {
        GraphBuf::Retired retired;
        GraphBuf words(&retired), queue(&retired);
        REQUIRE(grow(words, 1000) == 0 && words.cap() == 1125 && words.held_bytes() == 1125);
        REQUIRE(grow(words, 2000) == 0 && words.cap() == 2250);              // unmarked: the old block is freed
        REQUIRE(retired.empty() && CountingMem::live.size() == 1 && CountingMem::live_bytes == 2250);
        void *w1 = words.ptr();
        words.mark_in_graph();
        const size_t c0 = CountingMem::calls();
        REQUIRE(grow(words, 2250) == 0 && CountingMem::calls() == c0 && retired.empty());   // within capacity: nothing, marked or not
        REQUIRE(grow(words, 4000) == 0 && words.cap() == 4500 && words.ptr() != w1);
        REQUIRE(retired.size() == 1 && CountingMem::live.count(w1) == 1);    // marked: the old block lives on, and is counted
        REQUIRE(words.held_bytes() == 4500 + 2250 && CountingMem::live_bytes == 4500 + 2250);
        REQUIRE(grow(words, 8000) == 0 && retired.size() == 1);              // the mark went with the block: this growth frees
        REQUIRE(words.held_bytes() == 9000 + 2250 && CountingMem::live_bytes == 9000 + 2250);
        REQUIRE(grow(queue, 64) == 0 && queue.cap() == 72);
        queue.mark_in_graph();
        REQUIRE(grow(queue, 100) == 0 && queue.cap() == 112 && retired.size() == 2);
        REQUIRE(words.held_bytes() == 9000 + 2250 + 72 && CountingMem::live_bytes == 9000 + 2250 + 72 + 112);
        words.mark_in_graph();
        CountingMem::fail_next = true;                       // a marked buffer whose growth fails: retired all the same, then empty
        REQUIRE(grow(words, 20000) != 0 && words.ptr() == nullptr && words.cap() == 0 && retired.size() == 3);
        REQUIRE(words.held_bytes() == 9000 + 2250 + 72);
        words.release();                                     // the live block and the whole list
        REQUIRE(retired.empty() && words.held_bytes() == 0 && CountingMem::live_bytes == 112);
        queue.release();
        REQUIRE(CountingMem::live.empty());
        REQUIRE(grow(words, 10) == 0 && words.cap() == 11);  // usable afterwards
        words.mark_in_graph();
        REQUIRE(grow(words, 100) == 0 && retired.size() == 1);
        ++g_cases;
    }                                                        // destruction: live blocks and the list's
    REQUIRE(CountingMem::live.empty() && CountingMem::live_bytes == 0);

    // ---- the fixed-size owning pointer: frees on scope exit and on a second allocation; a borrowed block is never freed
    {
        Ptr p;
        REQUIRE(alloc_owned(p, 64) == 0 && p && CountingMem::live_bytes == 64);
        REQUIRE(alloc_owned(p, 32) == 0 && CountingMem::live_bytes == 32 && CountingMem::live.size() == 1);
        Ptr q = std::move(p);
        REQUIRE(!p && q && CountingMem::live.size() == 1);
        CountingMem::fail_next = true;
        REQUIRE(alloc_owned(q, 16) != 0 && !q && CountingMem::live.empty());
        unsigned mine[4] = {0, 1, 2, 3};
        const size_t f = CountingMem::frees;
        {
            Ptr b = borrowed<unsigned, CountingMem>(mine);
            REQUIRE(b.get() == mine);
            REQUIRE(alloc_owned(q, 8) == 0);
            b = std::move(q);                                // an owned block takes a borrowed one's place: nothing is freed ...
            REQUIRE(CountingMem::frees == f && CountingMem::live.size() == 1);
        }                                                    // ... and the owned one goes with its owner
        REQUIRE(CountingMem::frees == f + 1 && CountingMem::live.empty() && mine[3] == 3);
        ++g_cases;
    }
    REQUIRE(CountingMem::live.empty() && CountingMem::live_bytes == 0 && CountingMem::allocs >= CountingMem::frees);
    printf("buffers_driver: %d cases ok\n", g_cases);
    return 0;
}
