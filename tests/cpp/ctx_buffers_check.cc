// ctx_buffers_check.cc — host/ctx_buffers.h over a counting fake policy (tests/test_ctx_buffers.py compiles it with the
// address and undefined-behaviour sanitizers and runs it): when the owners allocate, when and in which order they free,
// what a failed allocation leaves, what a scope's end and a move leave.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "host/ctx_buffers.h"

namespace {

// malloc / free underneath; every call recorded as "+p", "-p" (pinned), "+d", "-d" (device) with its block; the n-th
// allocation from now on can be told to fail
struct Fake {
  struct Call { std::string what; void* p; size_t bytes; };
  static std::vector<Call> calls;
  static std::set<void*> live;
  static int fail_in;        // 1: the next allocation fails, 2: the one after it, ...; 0: none
  static int double_frees;
  static int Alloc(const char* what, void** p, size_t bytes, bool zero) {
    if (fail_in > 0 && --fail_in == 0) { calls.push_back({std::string(what) + " failed", nullptr, bytes}); return -2; }
    *p = std::malloc(bytes);
    std::memset(*p, zero ? 0 : 0xAB, bytes);   // (a pinned buffer comes as it comes)
    live.insert(*p);
    calls.push_back({what, *p, bytes});
    return 0;
  }
  static void Free(const char* what, void* p) {
    if (!live.erase(p)) { ++double_frees; return; }
    calls.push_back({what, p, 0});
    std::free(p);
  }
  static int PinAlloc(void** p, size_t bytes) { return Alloc("+p", p, bytes, false); }
  static void PinFree(void* p) { Free("-p", p); }
  static int DevAlloc(void** p, size_t bytes) { return Alloc("+d", p, bytes, true); }
  static void DevFree(void* p) { Free("-d", p); }
  static void Clear() { calls.clear(); fail_in = 0; }
  static std::string Trace() { std::string t; for (const Call& c : calls) t += c.what + " "; return t; }
};
std::vector<Fake::Call> Fake::calls;
std::set<void*> Fake::live;
int Fake::fail_in = 0;
int Fake::double_frees = 0;

int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s   [%s]\n", __LINE__, #cond, Fake::Trace().c_str()); ++g_failures; } } while (0)

template <class Buf>
void GrowSequence(const char* plus, const char* minus, bool alloc_first) {
  Fake::Clear();
  {
    Buf b;
    CHECK(b == nullptr && b.cap() == 0);
    CHECK(b.Ensure(0) == 0 && Fake::calls.empty() && b == nullptr);            // nothing asked for, nothing made
    CHECK(b.Ensure(10, 0, alloc_first) == 0 && b.cap() == 10 && b != nullptr);
    CHECK(Fake::Trace() == std::string(plus) + " ");
    CHECK(Fake::calls[0].bytes == 10 * sizeof(double));
    void* first = b;
    CHECK(b.Ensure(10, 0, alloc_first) == 0 && b.Ensure(3, 0, alloc_first) == 0);   // the same, a smaller one: no call
    CHECK(Fake::calls.size() == 1 && b == first && b.cap() == 10);
    CHECK(b.Ensure(25, 0, alloc_first) == 0 && b.cap() == 25 && b != nullptr);      // a real growth
    const std::string grow = alloc_first ? std::string(plus) + " " + minus + " " : std::string(minus) + " " + plus + " ";
    CHECK(Fake::Trace() == std::string(plus) + " " + grow);
    CHECK(Fake::calls[alloc_first ? 2 : 1].p == first);                             // the superseded block, once
    CHECK(Fake::live.size() == 1);
    static_cast<double*>(b)[24] = 1.0;                                               // (the whole of it is the caller's)
  }
  CHECK(Fake::live.empty() && Fake::calls.size() == 4 && Fake::calls.back().what == minus);
}

template <class Buf>
void FailureAtEveryPosition(bool alloc_first) {
  for (int pos = 1; pos <= 3; ++pos) {   // the first allocation, the first growth, the second
    Fake::Clear();
    {
      Buf b;
      const size_t sizes[3] = {4, 9, 30};
      for (int i = 0; i < 3; ++i) {
        if (i + 1 == pos) {
          Fake::fail_in = 1;
          CHECK(b.Ensure(sizes[i], 0, alloc_first) != 0);
          CHECK(b == nullptr && b.cap() == 0);            // never half-set
          CHECK(Fake::live.empty());                      // and the superseded one is not kept either
          CHECK(b.Ensure(2, 0, alloc_first) == 0 && b != nullptr && b.cap() == 2);   // a later Ensure succeeds, even a small one
        }
        CHECK(b.Ensure(sizes[i], 0, alloc_first) == 0 && b.cap() == sizes[i]);
      }
    }
    CHECK(Fake::live.empty());
  }
}

using PinnedD = idto_host::Pinned<double, Fake>;
using GrownD = idto_host::Grown<double, Fake>;

}  // namespace

int main() {
  GrowSequence<PinnedD>("+p", "-p", false);
  GrowSequence<GrownD>("+d", "-d", false);
  GrowSequence<GrownD>("+d", "-d", true);    // made first, the old one freed behind it (tr_rows, the solve staging)
  FailureAtEveryPosition<PinnedD>(false);
  FailureAtEveryPosition<GrownD>(false);
  FailureAtEveryPosition<GrownD>(true);

  Fake::Clear();
  {  // a minimum capacity: honoured when the buffer is made, and then it serves every request up to it
    idto_host::Pinned<char, Fake> up;
    CHECK(up.Ensure(100, 4096) == 0 && up.cap() == 4096 && Fake::calls[0].bytes == 4096);
    CHECK(up.Ensure(4096, 4096) == 0 && Fake::calls.size() == 1);
    CHECK(up.Ensure(5000, 4096) == 0 && up.cap() == 5000 && Fake::calls.size() == 3);
    PinnedD many;
    CHECK(many.Ensure(0, 1) == 0 && many == nullptr && Fake::calls.size() == 3);   // (nothing asked for: nothing made)
    CHECK(many.Ensure(1, 1) == 0 && many.cap() == 1);
  }
  CHECK(Fake::live.empty());

  Fake::Clear();
  {  // a device Ensure zero-fills the whole buffer, a grown one again
    GrownD d;
    for (size_t n : {7u, 64u}) {
      CHECK(d.Ensure(n) == 0);
      bool zero = true;
      for (size_t i = 0; i < n; ++i) zero = zero && static_cast<double*>(d)[i] == 0.0;
      CHECK(zero);
      static_cast<double*>(d)[n - 1] = 3.0;
    }
  }
  CHECK(Fake::live.empty());

  Fake::Clear();
  {  // a moved-from object frees nothing; a move assignment frees what the target held
    GrownD a;
    CHECK(a.Ensure(5) == 0);
    void* pa = a;
    GrownD b(std::move(a));
    CHECK(a == nullptr && a.cap() == 0 && b == pa && b.cap() == 5 && Fake::calls.size() == 1);
    GrownD t;
    CHECK(t.Ensure(6) == 0);
    void* pt = t;
    t = std::move(b);
    CHECK(t == pa && b == nullptr && Fake::calls.size() == 3 && Fake::calls[2].what == "-d" && Fake::calls[2].p == pt);
    t = GrownD();   // (how idto_hip_destroy empties a context's buffers)
    CHECK(t == nullptr && t.cap() == 0 && Fake::live.empty() && Fake::calls.size() == 4);
  }
  CHECK(Fake::calls.size() == 4 && Fake::live.empty());

  Fake::Clear();
  {  // the pair: both or neither
    idto_host::GrownPair<Fake> g;
    CHECK(g.Ensure(8, 0) == 0 && g.dev.cap() == 8 && g.pin == nullptr);   // (no mirror asked for)
    Fake::fail_in = 2;   // the device side grows, the pinned side fails
    CHECK(g.Ensure(16, 16) != 0 && g.dev.cap() == 16 && g.pin == nullptr && g.pin.cap() == 0);
    const size_t before = Fake::calls.size();
    CHECK(g.Ensure(16, 16) == 0 && g.dev.cap() == 16 && g.pin.cap() == 16);   // the next call repairs it: the missing side alone
    CHECK(Fake::calls.size() == before + 1 && Fake::calls.back().what == "+p");
    Fake::fail_in = 1;   // the device side fails: the pinned side is not touched, the call fails
    CHECK(g.Ensure(32, 32) != 0 && g.dev == nullptr && g.dev.cap() == 0 && g.pin.cap() == 16);
    CHECK(g.Ensure(32, 32) == 0 && g.dev.cap() == 32 && g.pin.cap() == 32);
  }
  CHECK(Fake::live.empty());
  CHECK(Fake::double_frees == 0);

  if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
  std::printf("ok: ctx_buffers\n");
  return 0;
}
