// TEST-ONLY driver of the handle table's sub-kind (qdsp_amd/csrc/stream_op.h) against the fake synchronous HIP runtime
// (fake_hip_runtime.cpp), a program of its own built with -fsanitize=address,undefined: two handle types of one kind, one at the
// default sub-kind and one that names its own, are told apart both ways; a type of another kind takes neither; every one is a
// stream op; a type without a kSub registers and looks up at 0.
#include "../../qdsp_amd/csrc/stream_op.h"

#include <stdio.h>

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) { printf("FAIL line %d: %s\n", __LINE__, #x); return 1; } \
    } while (0)

using namespace qh;

namespace {

struct Plain : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;
};
struct Sub : StreamOp {
    static constexpr OpKind kKind = OpKind::Rs;
    static constexpr int kSub = 1;
};
struct Other : StreamOp {
    static constexpr OpKind kKind = OpKind::Hirs;
};

int64_t nothing(StreamOp*, const void*, int64_t, int64_t, void*, int64_t, hipStream_t) { return 0; }
template <class T>
int64_t nothing_t(T*, const void*, int64_t, int64_t, void*, int64_t, hipStream_t) {
    return 0;
}
template <class T>
void drop(T* d) {
    op_free(d, [] {});
}
template <class T>
T* make() {
    T* d = nullptr;
    void* h = nullptr;
    if (op_new<T, nothing_t<T>>(&d, &h, true, 0, 1, 4)) return nullptr;
    const hipError_t err = stream_op_init(d, 0, 1, 4, 1, 1);
    if (op_created<drop<T>>(&h, d, err)) return nullptr;
    return static_cast<T*>(h);
}

}  // namespace

int main() {
    static_assert(op_sub<Plain>::value == 0 && op_sub<Sub>::value == 1 && op_sub<Other>::value == 0, "kSub where declared, else 0");
    Plain* p = make<Plain>();
    Sub* s = make<Sub>();
    Other* o = make<Other>();
    CHECK(p && s && o);
    // the same kind with a different sub is refused both ways
    CHECK(as<Plain>(p) == p && as<Sub>(s) == s && as<Other>(o) == o);
    CHECK(!as<Sub>(p) && !as<Plain>(s));
    CHECK(!as<Other>(p) && !as<Other>(s) && !as<Plain>(o) && !as<Sub>(o));
    // the two functions themselves: the default argument is sub 0
    CHECK(stream_op_lookup(p, OpKind::Rs) == p && stream_op_lookup(p, OpKind::Rs, 0) == p && !stream_op_lookup(p, OpKind::Rs, 1));
    CHECK(stream_op_lookup(s, OpKind::Rs, 1) == s && !stream_op_lookup(s, OpKind::Rs) && !stream_op_lookup(s, OpKind::Rs, 2));
    CHECK(!stream_op_lookup(s, OpKind::Hirs, 1) && !stream_op_lookup(nullptr, OpKind::Rs, 1));
    // whatever the sub-kind, a live handle is a stream op (qdsp_hip_last_kernel, qdsp_hip_set_done_event)
    CHECK(as_stream_op(p) == p && as_stream_op(s) == s && as_stream_op(o) == o);
    // registering again under another sub moves the handle; unregistering takes it out under every one
    stream_op_register(p, OpKind::Rs, 1);
    CHECK(as<Sub>(p) != nullptr && !as<Plain>(p));
    stream_op_register(p, OpKind::Rs);
    CHECK(as<Plain>(p) == p && !as<Sub>(p));
    void* stale = s;
    drop(s);
    CHECK(!as<Sub>(stale) && !as<Plain>(stale) && !as_stream_op(stale));
    drop(as<Sub>(stale));                                    // a second destroy: a call with null
    drop(p);
    drop(o);
    (void)nothing;
    printf("subkind ok\n");
    return 0;
}
