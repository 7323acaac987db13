// Buf<T> of csrc/device_buffer.h without a GPU: the four mem_* functions are malloc / free with a count of the live allocations
// of each kind and a switch that makes the k-th allocation fail.  Built with the sanitizers and run as a program of its own by
// tests/test_device_buffer_cpu.py.  Prints "FAIL <what>" per failed check and "ok <failures>" as its last line.
#include "../../iterative_solvers_amd/csrc/device_buffer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

namespace {
std::set<void*> g_device, g_pinned;      // what is live, by the function that has to free it
int g_allocs = 0, g_fail_at = 0;         // allocations so far; the one that fails (1-based, 0: none)
int g_wrong_free = 0;                    // frees through the wrong function, or of memory that is not live
int g_failures = 0;
const char* g_last_what = nullptr;

bool fails_now() { return ++g_allocs == g_fail_at; }
int live() { return (int)(g_device.size() + g_pinned.size()); }
void arm(int k) { g_allocs = 0; g_fail_at = k; }
void check(bool ok, const char* what) { if (!ok) { std::printf("FAIL %s\n", what); ++g_failures; } }
}  // namespace

namespace mi355cg {
int mem_device_alloc(void** out, size_t bytes, bool zero, const char* what) {
    if (fails_now()) { g_last_what = what; return -3; }
    void* p = std::malloc(bytes ? bytes : 1);
    std::memset(p, zero ? 0 : 0xa5, bytes);
    g_device.insert(p);
    *out = p;
    return 0;
}
void mem_device_free(void* p) { if (g_device.erase(p) != 1) ++g_wrong_free; else std::free(p); }
int mem_pinned_alloc(void** out, size_t bytes, const char* what) {
    if (fails_now()) { g_last_what = what; return -3; }
    void* p = std::malloc(bytes ? bytes : 1);
    g_pinned.insert(p);
    *out = p;
    return 0;
}
void mem_pinned_free(void* p) { if (g_pinned.erase(p) != 1) ++g_wrong_free; else std::free(p); }
}  // namespace mi355cg

using mi355cg::Buf;

namespace {

// The build-then-swap pattern of the library: five buffers (one pinned) built by a function that returns on the first error.
struct Ws {
    Buf<double> base, part, red;
    Buf<double> red_h;      // pinned
    Buf<int> tab;
    int tag = 0;
};
int build_ws(Ws& w, int tag) {
    if (int rc = Buf<double>::device_zeroed(w.base, 100)) return rc;
    if (int rc = Buf<double>::device(w.part, 10)) return rc;
    if (int rc = Buf<double>::device(w.red, 4, "sums")) return rc;
    if (int rc = Buf<double>::pinned(w.red_h, 4)) return rc;
    if (int rc = Buf<int>::device(w.tab, 7)) return rc;
    w.tag = tag;
    return 0;
}
// what mg_batch_ensure does with it: a local object, returned on failure, moved into the owner on success
int replace_ws(Ws& installed, int tag) {
    Ws fresh;
    if (int rc = build_ws(fresh, tag)) return rc;
    installed = std::move(fresh);
    return 0;
}

void test_empty() {
    { Buf<double> b; check(b.get() == nullptr && !b, "an empty buffer is a null pointer"); b.reset(); }
    check(live() == 0 && g_wrong_free == 0 && g_allocs == 0, "an empty buffer frees nothing");
}

void test_reset_and_destruction() {
    arm(0);
    Buf<double> b;
    check(Buf<double>::device_zeroed(b, 8) == 0 && b.get() && live() == 1, "device_zeroed allocates");
    double s = 0;
    for (int i = 0; i < 8; ++i) s += b[i];
    check(s == 0.0, "device_zeroed zero-fills");
    b.reset();
    check(live() == 0 && !b, "reset frees");
    b.reset();
    check(live() == 0 && g_wrong_free == 0, "a second reset frees nothing");
    { Buf<int> c; check(Buf<int>::device(c, 3) == 0 && live() == 1, "device allocates"); }
    check(live() == 0 && g_wrong_free == 0, "destruction frees exactly once");
    { Buf<int> c; Buf<int>::device(c, 3); int* first = c; Buf<int>::device(c, 5); check(live() == 1 && c.get() != nullptr && g_device.count(first) == 0, "a second allocation releases the first"); }
    check(live() == 0 && g_wrong_free == 0, "... and destruction frees the second");
}

void test_moves() {
    arm(0);
    {
        Buf<double> a;
        Buf<double>::device(a, 4);
        double* pa = a;
        Buf<double> b(std::move(a));
        check(b.get() == pa && a.get() == nullptr && live() == 1, "move construction transfers ownership");
        Buf<double> c;
        Buf<double>::device(c, 4);
        double* pc = c;
        check(live() == 2, "two live buffers");
        c = std::move(b);
        check(c.get() == pa && b.get() == nullptr && live() == 1 && g_device.count(pc) == 0, "move assignment frees the target's old memory");
        Buf<double>& self = c;
        c = std::move(self);
        check(c.get() == pa && live() == 1, "self-move is harmless");
        std::swap(a, c);
        check(a.get() == pa && c.get() == nullptr && live() == 1, "swap exchanges two buffers");
        std::swap(a, c);
        check(c.get() == pa && a.get() == nullptr && live() == 1, "... and back");
    }
    check(live() == 0 && g_wrong_free == 0, "moved-from buffers free nothing");
    {
        std::vector<Buf<double>> v(3);
        Buf<double>::device(v[1], 2);
        v.resize(40);                            // reallocation moves the elements
        check(live() == 1 && v[1].get() != nullptr, "a vector of buffers keeps them through a reallocation");
    }
    check(live() == 0 && g_wrong_free == 0, "... and frees them once");
}

void test_pinned() {
    arm(0);
    {
        Buf<int> h;
        check(Buf<int>::pinned(h, 1) == 0 && g_pinned.size() == 1 && g_device.empty(), "pinned allocates pinned memory");
        *h = 7;
        check(h[0] == 7, "a pinned word reads back");
    }
    check(live() == 0 && g_wrong_free == 0, "a pinned buffer is freed with the pinned function");
}

void test_borrow() {
    arm(0);
    double mine[4] = {1, 2, 3, 4};
    {
        Buf<double> b;
        b.borrow(mine);
        check(b.get() == mine && b[2] == 3 && live() == 0, "borrow views memory");
        Buf<double> moved(std::move(b));
        check(moved.get() == mine && b.get() == nullptr, "a borrow moves as a borrow");
    }
    check(live() == 0 && g_wrong_free == 0 && mine[3] == 4, "borrow never frees");
    {
        Buf<double> b;
        Buf<double>::device(b, 4);
        b.borrow(mine);
        check(live() == 0 && b.get() == mine, "borrow drops what was owned before");
        b.reset();
        check(b.get() == nullptr && g_wrong_free == 0, "reset of a borrow frees nothing");
        b.borrow(mine);
        check(Buf<double>::device(b, 4) == 0 && live() == 1 && b.get() != mine, "an allocation replaces a borrow");
    }
    check(live() == 0 && g_wrong_free == 0, "... and is freed");
}

void test_failed_allocation() {
    arm(1);
    Buf<double> b;
    check(Buf<double>::device(b, 4, "my text") == -3 && !b && live() == 0, "a failed allocation leaves an empty buffer empty");
    check(g_last_what && !std::strcmp(g_last_what, "my text"), "the caller's message reaches the allocator");
    arm(0);
    Buf<double>::device(b, 4);
    double* held = b;
    arm(1);
    check(Buf<double>::pinned(b, 4) == -3 && b.get() == held && live() == 1, "a failed allocation leaves a full buffer as it was");
    arm(0);
}

void test_build_then_swap() {
    arm(0);
    Ws installed;
    check(replace_ws(installed, 1) == 0 && live() == 5 && installed.tag == 1, "the first workspace is installed");
    const double* base = installed.base;
    const int* tab = installed.tab;
    for (int k = 1; k <= 5; ++k) {
        arm(k);
        const int rc = replace_ws(installed, 100 + k);
        char what[96];
        std::snprintf(what, sizeof what, "failure at allocation %d: error returned, nothing leaked, the installed workspace untouched", k);
        check(rc == -3 && live() == 5 && installed.tag == 1 && installed.base.get() == base && installed.tab.get() == tab && g_wrong_free == 0, what);
    }
    arm(0);
    check(replace_ws(installed, 2) == 0 && live() == 5 && installed.tag == 2 && g_device.count((void*)base) == 0, "a complete workspace replaces the installed one, which is freed");
    for (int k = 1; k <= 5; ++k) {               // the same with nothing installed
        arm(k);
        { Ws w; check(build_ws(w, k) == -3, "a local workspace fails at allocation k"); }
        check(live() == 5, "... and leaves nothing behind once it dies");
    }
    arm(0);
}

}  // namespace

int main() {
    test_empty();
    test_reset_and_destruction();
    test_moves();
    test_pinned();
    test_borrow();
    test_failed_allocation();
    check(live() == 0, "nothing is live between the groups");
    test_build_then_swap();
    check(live() == 0 && g_wrong_free == 0, "the live counter is 0 at exit");
    std::printf("ok %d\n", g_failures);
    return g_failures ? 1 : 0;
}
