// own_check.cpp -- the handle owners (csrc/rt_own.h) over a counting stub, on the host alone:
// every handle created is destroyed once -- at scope exit, across moves, after a double
// reset -- a pool grows by whole groups or not at all, and an all-or-nothing set-up that
// fails half way leaves nothing alive.  Includes rt_own.h only.  Exit status 1 on a mismatch.
#include <cstdio>
#include <set>
#include <utility>

#include "rt_own.h"

namespace {

int bad = 0;
void expect(bool ok, const char* what)
{
    if (ok) return;
    std::printf("MISMATCH %s\n", what);
    bad++;
}

// handles are the addresses of heap ints (the sanitizer sees a leak or a double destroy too)
struct Stub {
    using type = int*;
    using status = int;
    static int created, destroyed, fail_at;   // fail_at: the creation (counted from 1) that fails, 0 for none
    static unsigned last_flags;
    static std::set<int*> live;
    static int create(int** out, unsigned flags)
    {
        last_flags = flags;
        if (fail_at && created + 1 == fail_at) {
            fail_at = 0;
            *out = reinterpret_cast<int*>(0x5A);   // (a failed create may leave rubbish: the owner must not keep it)
            return 7;
        }
        created++;
        *out = new int(created);
        live.insert(*out);
        return 0;
    }
    static void destroy(int* h)
    {
        expect(live.erase(h) == 1, "destroy of a handle that is not alive");
        destroyed++;
        delete h;
    }
    static bool balanced() { return created == destroyed && live.empty(); }
};
int Stub::created = 0, Stub::destroyed = 0, Stub::fail_at = 0;
unsigned Stub::last_flags = 0;
std::set<int*> Stub::live;

using H = Handle<Stub>;

// what RT_OPT_ASYNC_FOLD does: six handles into locals, moved into place when all exist
struct Six {
    H stream, ev[5];
};
int setup_six(Six& s)
{
    H st, ev[5];
    if (int e = st.ensure()) return e;
    for (H& x : ev)
        if (int e = x.ensure(2u)) return e;
    s.stream = std::move(st);
    for (int i = 0; i < 5; i++) s.ev[i] = std::move(ev[i]);
    return 0;
}

}  // namespace

int main()
{
    {   // lazy, flags, idempotent ensure, scope exit
        H a;
        expect(!a && a.get() == nullptr && Stub::created == 0, "a new owner holds nothing");
        expect(a.ensure(2u) == 0 && a && Stub::created == 1 && Stub::last_flags == 2u, "ensure creates with its flags");
        int* const first = a.get();
        expect(a.ensure() == 0 && a.get() == first && Stub::created == 1, "a second ensure keeps the handle");
    }
    expect(Stub::balanced() && Stub::created == 1, "scope exit");
    {   // moves: construction, assignment over a live handle, self-assignment
        H a, b;
        a.ensure();
        b.ensure();
        int* const pa = a.get();
        H c(std::move(a));
        expect(!a && c.get() == pa, "move construction empties the source");
        b = std::move(c);
        expect(!c && b.get() == pa && Stub::destroyed == 2, "move assignment destroys what it overwrites");
        H& alias = b;
        b = std::move(alias);
        expect(b.get() == pa && Stub::destroyed == 2, "self-assignment keeps the handle");
    }
    expect(Stub::balanced() && Stub::created == 3, "after moves");
    {   // double reset, and a failed creation
        H a;
        a.ensure();
        a.reset();
        a.reset();
        expect(!a && Stub::balanced(), "double reset");
        Stub::fail_at = Stub::created + 1;
        expect(a.ensure() == 7 && !a && a.get() == nullptr, "a failed ensure leaves the owner empty");
        expect(a.ensure() == 0 && a, "and the next one creates");
    }
    expect(Stub::balanced() && Stub::created == 5, "after resets");
    {   // a pool of triples, at most two of them
        Pool<Stub, 3, 6> p;
        expect(!p.full() && p.ensure_group() == 0 && p.h.size() == 3, "the first group");
        expect(p.ensure_group() == 0 && p.h.size() == 3 && Stub::created == 8, "a group that exists is not made again");
        p.used = 3;
        Stub::fail_at = Stub::created + 2;   // the second handle of the second group
        expect(p.ensure_group() == 7 && p.h.size() == 3, "a failed growth leaves whole groups");
        expect(Stub::created - Stub::destroyed == 3, "and destroys the part it made");
        expect(p.ensure_group() == 0 && p.h.size() == 6 && p[3] && p[5], "the growth after it succeeds");
        p.used = 6;
        expect(p.full(), "the cap");
        int* const h0 = p[0];
        p.used = 0;   // a reset reuses the handles
        expect(!p.full() && p.ensure_group() == 0 && p[0] == h0 && p.h.size() == 6, "reuse after a reset");
        Pool<Stub, 3, 6> q(std::move(p));
        expect(q[0] == h0 && q.h.size() == 6, "a moved pool");
    }
    expect(Stub::balanced() && Stub::created == 12, "after the pool");
    {   // all or nothing: six handles whose fourth fails
        Six s;
        Stub::fail_at = Stub::created + 4;
        expect(setup_six(s) == 7, "the set-up reports the failure");
        bool none = !s.stream;
        for (H& x : s.ev) none = none && !x;
        expect(none && Stub::balanced(), "a failed set-up leaves none alive and its target untouched");
        expect(setup_six(s) == 0 && s.stream && s.ev[4] && Stub::created - Stub::destroyed == 6, "the set-up after it succeeds");
    }
    expect(Stub::balanced() && Stub::created == 21, "after the set-ups");
    std::printf("own_check: %d mismatches (%d created, %d destroyed)\n", bad, Stub::created, Stub::destroyed);
    return bad ? 1 : 0;
}
