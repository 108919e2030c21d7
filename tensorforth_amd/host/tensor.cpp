// tensor.cpp - backend bring-up, HBM arena, object store and the Tensor methods.
// Semantics follow the reference's Tensor (src/mu/tensor.cu) and MMU (src/mu/mmu.cu) including
// their quirks (std() = sqrt(sum)/numel, SCALAR() LSB clearing, small-sum host loop); every
// device operation goes through the t4k_* C-ABI.
#include "t4.h"
#include <stdarg.h>
#include <stdlib.h>
#include <time.h>
#include <algorithm>

namespace t4 {

const char *LAYER_NAME[] = { "output ", "conv2d ", "linear ", "flatten", "relu   ", "tanh   ", "sigmoid", "selu   ",
                             "leakyrl", "elu    ", "dropout", "softmax", "logsmax", "avgpool", "maxpool", "minpool",
                             "batchnm", "upsampl", "dconv2d", "attentn", "addnorm", "embed  " };        // (attentn, addnorm, embed: beyond the reference's list)

static bool g_ready = false;
static float *g_scalar = nullptr;       // device scratch for reductions (replaces Tensor::_tmp)
static int   *g_iscalar = nullptr;

void die_if_no_backend() {
    if (g_ready) return;
    const char *dev = getenv("T4_DEVICE");
    int rc = t4k_init(dev ? atoi(dev) : 0);
    if (rc != T4K_OK) {
        fprintf(stderr, "tensorForth: GPU backend unavailable (%s): %s\n", t4k_backend_name(), t4k_last_error());
        exit(2);                         // the product path has no CPU fallback
    }
    const char *seed = getenv("T4_SEED");
    t4k_rand_init(seed ? strtoull(seed, 0, 10) : (uint64_t)time(NULL));     // reference seeds from time(), sys.cpp:37
    void *p = nullptr;
    t4k_malloc(&p, 256); g_scalar = (float *)p; g_iscalar = (int *)(g_scalar + 16);
    g_ready = true;
}
static void (*g_sink)(const char *, void *) = nullptr;
static void *g_sink_user = nullptr;
void set_host_sink(void (*fn)(const char *, void *), void *user) { g_sink = fn; g_sink_user = user; }
void get_host_sink(void (**fn)(const char *, void *), void **user) { *fn = g_sink; *user = g_sink_user; }
void hprintf(const char *fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    if (g_sink) g_sink(buf, g_sink_user); else fputs(buf, stdout);
}
void hputs(const std::string &text) { if (g_sink) g_sink(text.c_str(), g_sink_user); else fputs(text.c_str(), stdout); }   // text of any length (hprintf formats into 1 KiB)
int chk(int rc, const char *what) {
    if (rc != T4K_OK) hprintf("%s failed: %s\n", what, t4k_last_error());     // print-and-continue (ten4_types.h:25)
    return rc;
}
t4k_stream_t stream() { return nullptr; }

// ---------------------------------------------------------------- Arena
Arena &Arena::get() { static Arena a; return a; }
void Arena::add_slab(size_t need) {
    die_if_no_backend();
    size_t sz = (size_t)256 << 20;                       // 256 MiB slabs; 288 GB of HBM leaves room to grow
    const char *e = getenv("T4_SLAB_MB"); if (e) sz = (size_t)atol(e) << 20;
    while (sz < need) sz <<= 1;
    void *p = nullptr;
    if (chk(t4k_malloc(&p, sz), "arena slab")) { fprintf(stderr, "out of HBM\n"); exit(3); }
    slabs_.push_back({(char *)p, sz});
    put_free((char *)p, sz);
}
// Free blocks are kept twice: by address (coalescing with the neighbours on free) and by size (best fit in O(log n) on alloc - the
// reference's TLSF gives O(1); a `matmul drop` loop or a training script allocates and frees a tensor per word).  No headers live in
// device memory: everything here is host-side bookkeeping over 256 MiB hipMalloc slabs.
void Arena::put_free(char *p, size_t sz) { free_[p] = sz; by_size_.insert({sz, p}); }
void Arena::take_free(std::map<char *, size_t>::iterator it) { by_size_.erase({it->second, it->first}); free_.erase(it); }
float *Arena::alloc(size_t nfloat) {
    const size_t need = ((nfloat ? nfloat : 1) * sizeof(float) + 255) & ~(size_t)255;
    for (int pass = 0; pass < 2; pass++) {
        auto fit = by_size_.lower_bound({need, nullptr});  // smallest block that fits (lowest address among equals)
        if (fit != by_size_.end()) {
            char *p = fit->second; const size_t rest = fit->first - need;
            take_free(free_.find(p));
            if (rest) put_free(p + need, rest);
            blocks_[p] = need; used_ += need; peak_ = std::max(peak_, used_);
            return (float *)p;
        }
        add_slab(need);
    }
    return nullptr;
}
void Arena::free(float *fp) {
    char *p = (char *)fp;
    auto b = blocks_.find(p);
    if (b == blocks_.end()) return;
    size_t sz = b->second; blocks_.erase(b); used_ -= sz;
    auto same_slab = [this](char *a, char *c) { for (auto &s : slabs_) if (a >= s.base && a < s.base + s.size) return c >= s.base && c < s.base + s.size; return false; };
    auto nx = free_.lower_bound(p);
    if (nx != free_.end() && p + sz == nx->first && same_slab(p, nx->first)) { sz += nx->second; auto dead = nx++; take_free(dead); }   // merge with next
    if (nx != free_.begin()) {
        auto pv = std::prev(nx);
        if (pv->first + pv->second == p && same_slab(pv->first, p)) { p = pv->first; sz += pv->second; take_free(pv); }                 // merge with previous
    }
    put_free(p, sz);
}

// ---------------------------------------------------------------- Store
Store &Store::get() { static Store s; return s; }
int Store::put(Obj *o) {
    int id;
    if (!free_ids_.empty()) { id = free_ids_.back(); free_ids_.pop_back(); objs_[id] = o; }
    else { id = (int)objs_.size(); objs_.push_back(o); }
    o->id = id; nlive_++;
    return id;
}
void Store::release(Obj *o) { objs_[o->id] = nullptr; free_ids_.push_back(o->id); nlive_--; delete o; }
Obj &Store::du2obj(DU v) {
    Obj *o = objs_[du_bits(v) >> 2];
    if (o && o->type == T_TENSOR && ((Tensor *)o)->stale_owner) ((Tensor *)o)->stale_owner->materialize_dx0();   // a lazily skipped dX: produce it before anybody looks
    return *o;
}
DU   Store::obj2du(Obj &o) { return bits_du(((uint32_t)o.id << 2) | 1u); }

Tensor &Store::tensor(uint64_t sz) {
    Tensor *t = new Tensor();
    t->type = T_TENSOR; t->numel = sz; t->rank = 1;
    t->shape[0] = (uint32_t)sz; t->shape[1] = t->shape[2] = t->shape[3] = 1;
    t->data = Arena::get().alloc(sz);
    put(t);
    return *t;
}
Tensor &Store::tensor(uint32_t h, uint32_t w) { Tensor &t = tensor((uint64_t)h * w); t.reshape(h, w); return t; }
Tensor &Store::tensor(uint32_t n, uint32_t h, uint32_t w, uint32_t c) {
    Tensor &t = tensor((uint64_t)n * h * w * c); t.reshape(n, h, w, c); return t;
}
Tensor &Store::copy(Tensor &t0) {                       // MMU::copy src/mu/mmu.cu:273-295
    Tensor &t1 = tensor(t0.numel);
    t1.rank = t0.rank; memcpy(t1.shape, t0.shape, sizeof(t0.shape)); memcpy(t1.stride, t0.stride, sizeof(t0.stride));
    t1.iparm = t0.iparm; t1.xparm = t0.xparm;
    t1 = t0;
    return t1;
}
Tensor &Store::dim(Tensor &t0) {                        // MMU::dim mmu.cu:296-302: HWCN -> NHWC
    const int map[] = {3, 0, 1, 2};
    Tensor &t = tensor(4);
    float v[4]; for (int i = 0; i < 4; i++) v[i] = (float)t0.shape[map[i]];
    t.from_host(v, 4);
    return t;
}
#pragma weak t4k_window
Tensor &Store::slice(Tensor &t0, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1) {   // mmu.cu:307-330
    if (t0.rank < 2) { hprintf("dim?"); return t0; }
    if (x1 == (uint32_t)-1) x1 = t0.W();
    if (y1 == (uint32_t)-1) y1 = t0.H();
    Tensor &t1 = t0.rank == 2 ? tensor(y1 - y0, x1 - x0) : tensor(t0.N(), y1 - y0, x1 - x0, t0.C());
    if (t4k_window && x0 < x1 && x1 <= t0.W() && y0 < y1 && y1 <= t0.H()) {   // a valid window: one launch in place of a memcpy per (sample, row)
        const int soff[4] = { 0, (int)y0, (int)x0, 0 }, doff[4] = { 0, 0, 0, 0 }, ext[4] = { (int)t1.N(), (int)t1.H(), (int)t1.W(), (int)t1.C() };
        Tensor::window(t0, soff, t1, doff, ext);
        return t1;
    }
    const uint32_t N = t1.N(), C = t1.C();
    const size_t bsz = sizeof(float) * C * t1.W();
    for (uint32_t n = 0; n < N; n++)
        for (uint32_t j = y0, j0 = 0; j < y1; j++, j0++)
            t4k_memcpy_d2d(t1.slice(n) + (size_t)C * j0 * t1.W(), t0.slice(n) + (size_t)C * (j * t0.W() + x0), bsz, stream());
    return t1;
}
void Store::free(Tensor &t) {                           // MMU::free mmu.cu:247-268
    if (t.owns && t.data) Arena::get().free(t.data);
    if (t.grad_fn != 0) {
        for (int i = 0; i < 4 && t.mtum[i]; i++) { if (t.mtum[i] == t.grad[i]) continue; free(*t.mtum[i]); }
        if (t.mtum[4]) free(*t.mtum[4]);
        for (int i = 0; i < 4; i++) if (t.grad[i]) free(*t.grad[i]);
        if (t.grad[4]) free(*t.grad[4]);
    }
    release(&t);
}
void Store::drop(Obj &o) {
    if (o.type == T_MODEL) { ((Model &)o).free_all(); release(&o); return; }
    if (o.type == T_DATASET) {
        Dataset &d = (Dataset &)o;
        if (d.cp) d.cp->idle();
        d.release_ring();
        d.data = nullptr; d.owns = false;
        release(&o); return;
    }
    free((Tensor &)o);
}
void Store::mark_free(DU v) { if (!IS_VIEW(v)) marked_.push_back(v); }
void Store::sweep() {
    for (DU v : marked_) { uint32_t id = du_bits(v) >> 2; if (id < objs_.size() && objs_[id]) drop(*objs_[id]); }
    marked_.clear();
}

// ---------------------------------------------------------------- Tensor
Tensor &Tensor::reshape(uint64_t sz) {
    if (sz == numel) { rank = 1; shape[0] = (uint32_t)sz; shape[1] = shape[2] = shape[3] = 1; stride[0] = stride[1] = stride[2] = stride[3] = 1; }
    else hprintf("  tensor#reshape sz != numel (%ld != %ld)\n", (long)sz, (long)numel);
    return *this;
}
Tensor &Tensor::reshape(uint32_t h, uint32_t w) {
    if ((uint64_t)h * w == numel) { rank = 2; shape[0] = h; shape[1] = w; shape[2] = shape[3] = 1; }
    else hprintf("  tensor#reshape sz != numel (%ld != %ld)\n", (long)((uint64_t)h * w), (long)numel);
    return *this;
}
Tensor &Tensor::reshape(uint32_t n, uint32_t h, uint32_t w, uint32_t c) {
    if ((uint64_t)n * h * w * c == numel) { rank = 4; shape[0] = h; shape[1] = w; shape[2] = c; shape[3] = n; }
    else hprintf("  tensor#reshape sz != numel (%ld != %ld)\n", (long)((uint64_t)n * h * w * c), (long)numel);
    return *this;
}
Tensor &Tensor::zeros() { chk(t4k_memset(data, 0, sizeof(float) * numel, stream()), "zeros"); return *this; }
Tensor &Tensor::map(int op, DU v) { chk(t4k_math(op, data, v, (long)numel, stream()), "map"); return *this; }
Tensor &Tensor::identity() { for (uint32_t n = 0; n < N(); n++) chk(t4k_identity(slice(n), H(), W(), C(), stream()), "identity"); return *this; }
Tensor &Tensor::normalize(DU avg, DU std) {             // tensor.cu:573-578
    t4k_ts_op(T4K_SUB, data, avg, data, (long)numel, stream());
    t4k_ts_op(T4K_DIV, data, std, data, (long)numel, stream());
    return *this;
}
Tensor &Tensor::operator=(Tensor &t) { chk(t4k_copy(t.data, data, (long)std::min(numel, t.numel), stream()), "copy"); return *this; }

static DU read_scalar() { DU v = 0; t4k_memcpy_d2h(&v, g_scalar, sizeof(DU), stream()); t4k_sync(stream()); return v; }

DU Tensor::sum() {                                      // tensor.cu:224-236
    chk(t4k_reduce(T4K_RED_SUM, data, (long)numel, 0, g_scalar, stream()), "sum");    // every size on the device (the reference sums short tensors on the host)
    DU v = read_scalar();
    return SCALAR(v);
}
DU Tensor::avg() { DU v = sum() / numel; return SCALAR(v); }
DU Tensor::std() {                                      // sqrt(sum (x-avg)^2) / numel   (tensor.cu:242-250)
    DU mx = avg();
    t4k_reduce(T4K_RED_NVAR, data, (long)numel, mx, g_scalar, stream());
    DU v = read_scalar(); v = numel ? sqrtf(v) / numel : 0.0f;
    return SCALAR(v);
}
DU Tensor::norm() { t4k_reduce(T4K_RED_NVAR, data, (long)numel, 0, g_scalar, stream()); DU v = sqrtf(read_scalar()); return SCALAR(v); }
DU Tensor::max()  { t4k_reduce(T4K_RED_MAX, data, (long)numel, 0, g_scalar, stream()); DU v = read_scalar(); return SCALAR(v); }
DU Tensor::min()  { t4k_reduce(T4K_RED_MIN, data, (long)numel, 0, g_scalar, stream()); DU v = read_scalar(); return SCALAR(v); }
DU Tensor::dot(Tensor &B) {
    if (rank == 1 && B.rank == 1 && numel == B.numel) t4k_dot(data, B.data, g_scalar, 1.0f, 0.0f, (int)numel, 1, stream());
    else hprintf("A.dot(B) dim? %ld != %ld)\n", (long)numel, (long)B.numel);
    DU v = read_scalar(); return SCALAR(v);
}
DU Tensor::loss(Loss op, Tensor &tgt) {                 // tensor.cu:288-325
    DU z = 0;
    switch (op) {
    case LOSS_MSE: ten_op(T4K_SUB, *this, tgt, *this); ten_op(T4K_MUL, *this, *this, *this); z = sum(); break;
    case LOSS_BCE: t4k_bce(tgt.data, data, (long)numel, g_scalar, stream()); z = -read_scalar(); break;
    case LOSS_CE:  map(T4K_LN);                         /* fall through */
    case LOSS_NLL: ten_op(T4K_MUL, *this, tgt, *this); z = -sum(); break;
    default: hprintf("Model#loss op=%d not supported!\n", op);
    }
    z /= N();
    return SCALAR(z);
}
uint32_t Tensor::has_nan() {
    t4k_nan_inf(data, (long)numel, g_iscalar, stream());
    int c = 0; t4k_memcpy_d2h(&c, g_iscalar, sizeof(int), stream()); t4k_sync(stream());
    return (uint32_t)c;
}
void Tensor::to_host(std::vector<float> &h, uint64_t n) {
    if (!n || n > numel) n = numel;
    h.resize(n);
    if (n) { t4k_memcpy_d2h(h.data(), data, n * sizeof(float), stream()); t4k_sync(stream()); }
}
void Tensor::from_host(const float *h, uint64_t n, uint64_t off) {
    if (off + n > numel) n = off < numel ? numel - off : 0;
    if (n) { t4k_memcpy_h2d(data + off, h, n * sizeof(float), stream()); t4k_sync(stream()); }
}
DU Tensor::get(uint64_t i) { DU v = 0; if (i < numel) { t4k_memcpy_d2h(&v, data + i, sizeof(DU), stream()); t4k_sync(stream()); } return v; }
void Tensor::set(uint64_t i, DU v) { if (i < numel) { t4k_memcpy_h2d(data + i, &v, sizeof(DU), stream()); t4k_sync(stream()); } }

Tensor &Tensor::ten_op(int op, Tensor &A, DU v, Tensor &O) {     // tensor.cu:16-23
    chk(t4k_ts_op(op, A.data, v, O.data, (long)A.numel, stream()), "ten_op");
    return O;
}
#pragma weak t4k_tt_op_bcast
#pragma weak t4k_transpose_batched
Tensor &Tensor::ten_op(int op, Tensor &A, Tensor &B, Tensor &O) {   // tensor.cu:28-53 (N broadcast)
    const uint32_t Na = A.N(), Nb = B.N(), N = std::max(Na, Nb);
    if (A.HWC() != B.HWC() || (Na == 1 ? B.numel : A.numel) != O.numel) {
        hprintf("  tensor#ten_op A.HWC(%ld)!=B.HWC(%ld) or N, C diff\n", (long)A.HWC(), (long)B.HWC());
        return O;
    }
    if ((Na == 1 || Nb == 1) && Na != Nb) {
        const long hwc = (long)A.HWC();
        if (t4k_tt_op_bcast && hwc <= 0x7fffffffL) {     // one launch for the whole batch (the same values as the loop below)
            const int dim[4] = { (int)N, 1, 1, (int)hwc };
            const long sA[4] = { Na == 1 ? 0 : hwc, 0, 0, 1 }, sB[4] = { Nb == 1 ? 0 : hwc, 0, 0, 1 };
            chk(t4k_tt_op_bcast(op, A.data, B.data, O.data, dim, sA, sB, stream()), "ten_op");
            return O;
        }
        for (uint32_t n = 0; n < N; n++)
            t4k_tt_op(op, A.slice(Na == 1 ? 0 : n), B.slice(Nb == 1 ? 0 : n), O.slice(n), (long)A.HWC(), stream());
    } else chk(t4k_tt_op(op, A.data, B.data, O.data, (long)A.numel, stream()), "ten_op");
    return O;
}
// NumPy broadcasting for + - * / beyond ten_op (tenvm.cpp:277-287 gives NumPy as the meaning of the tensor operators):
// O[n,h,w,c] = A[..] op B[..], an operand's axis of extent 1 serving every index of O's.  O has the axis-wise maximum shape (the caller
// checked that the extents agree or are 1).  One t4k_tt_op_bcast launch; the symbol is referenced weakly, and over a C-ABI without it
// (the CPU oracle) each broadcast operand is first expanded into a temporary of O's shape, innermost axis first - t4k_broadcast_rows
// where nothing lies inside the axis, copies of the inner block otherwise - and one t4k_tt_op does the arithmetic.
static void nhwc_of(Tensor &T, long e[4]) { e[0] = T.N(); e[1] = T.H(); e[2] = T.W(); e[3] = T.C(); }
static Tensor *expand_to(Tensor &X, const long dim[4]) {  // nullptr: X has O's shape already
    long cur[4]; nhwc_of(X, cur);
    Tensor *have = nullptr;
    float *src = X.data;
    for (int k = 3; k >= 0; k--) {
        if (cur[k] == dim[k]) continue;                  // cur[k] == 1 < dim[k]
        long outer = 1, inner = 1;
        for (int i = 0; i < k; i++) outer *= cur[i];
        for (int i = k + 1; i < 4; i++) inner *= cur[i];
        const long D = dim[k];
        Tensor &T = Store::get().tensor((uint64_t)(outer * D * inner));
        if (inner == 1) chk(t4k_broadcast_rows(src, T.data, (int)outer, (int)D, stream()), "broadcast_rows");
        else for (long o = 0; o < outer; o++) for (long d = 0; d < D; d++)
            chk(t4k_copy(src + o * inner, T.data + (o * D + d) * inner, inner, stream()), "copy");
        if (have) Store::get().free(*have);
        have = &T; src = T.data; cur[k] = D;
    }
    return have;
}
Tensor &Tensor::ten_bcast(int op, Tensor &A, Tensor &B, Tensor &O) {
    long ea[4], eb[4], eo[4]; nhwc_of(A, ea); nhwc_of(B, eb); nhwc_of(O, eo);
    if (t4k_tt_op_bcast) {
        int dim[4]; long sA[4], sB[4], da = 1, db = 1;
        for (int i = 3; i >= 0; i--) {
            dim[i] = (int)eo[i];
            sA[i] = ea[i] == 1 ? 0 : da; da *= ea[i];
            sB[i] = eb[i] == 1 ? 0 : db; db *= eb[i];
        }
        chk(t4k_tt_op_bcast(op, A.data, B.data, O.data, dim, sA, sB, stream()), "ten_bcast");
        return O;
    }
    Tensor *Ta = expand_to(A, eo), *Tb = expand_to(B, eo);
    chk(t4k_tt_op(op, Ta ? Ta->data : A.data, Tb ? Tb->data : B.data, O.data, (long)O.numel, stream()), "ten_bcast");
    if (Ta) Store::get().free(*Ta);
    if (Tb) Store::get().free(*Tb);
    return O;
}
// The walk of the two fallbacks below, over a C-ABI without the axis entries (the CPU oracle): T is viewed as (N,H,W,C); for every index of
// the unmasked axes, in output order, the elements along the masked axes (one group) are gathered into a temporary row with t4k_copy - the
// trailing masked axes are one contiguous copy - and f(row, elements, group index) runs; with `back` the row is then copied to where it came from.
template <typename F>
static void for_each_group(Tensor &T, int mask, bool back, F f) {
    long e[4]; nhwc_of(T, e);
    bool red[4]; long str[4], d = 1, cnt = 1;
    for (int i = 3; i >= 0; i--) { red[i] = (mask & (8 >> i)) != 0; str[i] = d; d *= e[i]; if (red[i]) cnt *= e[i]; }
    int tail = 4; long run = 1;                          // the trailing masked axes are one contiguous run
    while (tail > 0 && (red[tail - 1] || e[tail - 1] == 1)) { run *= e[tail - 1]; tail--; }
    Tensor &tmp = Store::get().tensor((uint64_t)cnt);
    long k[4], r[4], o = 0, Rn[4];                       // k: the group's index, r: the masked axes' (both 0 where the other walks)
    const long K[4] = { red[0] ? 1 : e[0], red[1] ? 1 : e[1], red[2] ? 1 : e[2], red[3] ? 1 : e[3] };
    for (int i = 0; i < 4; i++) Rn[i] = (i < tail && red[i]) ? e[i] : 1;
    for (k[0] = 0; k[0] < K[0]; k[0]++) for (k[1] = 0; k[1] < K[1]; k[1]++) for (k[2] = 0; k[2] < K[2]; k[2]++) for (k[3] = 0; k[3] < K[3]; k[3]++, o++)
        for (int pass = 0; pass < (back ? 2 : 1); pass++) {   // gather, f, scatter
            long at = 0;
            for (r[0] = 0; r[0] < Rn[0]; r[0]++) for (r[1] = 0; r[1] < Rn[1]; r[1]++) for (r[2] = 0; r[2] < Rn[2]; r[2]++) for (r[3] = 0; r[3] < Rn[3]; r[3]++, at += run) {
                long off = 0;
                for (int i = 0; i < 4; i++) off += (k[i] + r[i]) * str[i];
                if (pass) chk(t4k_copy(tmp.data + at, T.data + off, run, stream()), "copy");
                else      chk(t4k_copy(T.data + off, tmp.data + at, run, stream()), "copy");
            }
            if (!pass) f(tmp.data, cnt, o);
        }
    Store::get().free(tmp);
}
// Axis reductions (beyond the reference, whose sum / avg / std / norm fold a whole tensor: tensor.cu:224-250): T is viewed
// as (N,H,W,C) - a matrix (1,H,W,1), a vector the column (1,K,1,1) - and R has T's rank with every masked axis at extent 1.  One
// t4k_reduce_axes launch (two for few outputs behind long reductions) plus the element-wise sqrt / division of the word: a count
// that no extent changes, and no scalar is read back.  The symbol is referenced weakly: over a C-ABI without it (the CPU oracle)
// every output element gathers what it folds (for_each_group) and takes one t4k_reduce written straight to its place.
#pragma weak t4k_reduce_axes
static void reduce_into(int red_op, Tensor &T, int mask, Tensor *center, Tensor &R) {
    if (t4k_reduce_axes) {
        long e[4]; nhwc_of(T, e);
        const int dim[4] = { (int)e[0], (int)e[1], (int)e[2], (int)e[3] };
        chk(t4k_reduce_axes(red_op, T.data, R.data, dim, mask, center ? center->data : nullptr, stream()), "reduce_axes");
        return;
    }
    for_each_group(T, mask, false, [&](float *row, long cnt, long o) {
        chk(t4k_reduce(red_op, row, cnt, center ? center->get((uint64_t)o) : 0.0f, R.data + o, stream()), "reduce");
    });
}
Tensor &Tensor::reduce_axes(int word, Tensor &T, int mask) {
    long e[4], cnt = 1; nhwc_of(T, e);
    for (int i = 0; i < 4; i++) if (mask & (8 >> i)) { cnt *= e[i]; e[i] = 1; }
    auto result = [&]() -> Tensor & {
        return T.rank == 4 ? Store::get().tensor((uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3])
             : T.rank == 2 ? Store::get().tensor((uint32_t)e[1], (uint32_t)e[2]) : Store::get().tensor((uint64_t)e[1]);
    };
    Tensor &R = result();
    switch (word) {
    case AX_SUM:  reduce_into(T4K_RED_SUM, T, mask, nullptr, R); break;
    case AX_AVG:  reduce_into(T4K_RED_SUM, T, mask, nullptr, R); ten_op(T4K_DIV, R, (DU)cnt, R); break;            // sum / cnt: one fp32 division, as Tensor::avg
    case AX_NORM: reduce_into(T4K_RED_NVAR, T, mask, nullptr, R); R.map(T4K_SQRT); break;
    case AX_STD: {                                       // sqrt(sum (x - avg)^2) / cnt, avg the fp32 tensor `avg` returns (Tensor::std, tensor.cu:242-250)
        Tensor &A = reduce_axes(AX_AVG, T, mask);
        reduce_into(T4K_RED_NVAR, T, mask, &A, R);
        R.map(T4K_SQRT); ten_op(T4K_DIV, R, (DU)cnt, R);
        Store::get().free(A);
    } break;
    }
    return R;
}
// Axis softmax (beyond the reference, whose `softmax` word treats the whole tensor as one distribution: netvm.cpp:36-39):
// T, viewed as (N,H,W,C) like the axis reductions above, is rewritten in place - for every index of the unmasked axes the elements along
// the masked axes become exp(x - max) / sum exp(x - max).  One t4k_softmax_axes call, nothing read back.  The symbol is referenced
// weakly: over a C-ABI without it (the CPU oracle) every group is gathered into a temporary row (for_each_group), taken through
// t4k_softmax(row, row, 1, len) and copied back.
#pragma weak t4k_softmax_axes
void Tensor::softmax_axes(Tensor &T, int mask) {
    if (t4k_softmax_axes) {
        long e[4]; nhwc_of(T, e);
        const int dim[4] = { (int)e[0], (int)e[1], (int)e[2], (int)e[3] };
        chk(t4k_softmax_axes(T.data, T.data, dim, mask, stream()), "softmax_axes");
        return;
    }
    for_each_group(T, mask, true, [&](float *row, long cnt, long) { chk(t4k_softmax(row, row, 1, (int)cnt, stream()), "softmax"); });
}
Tensor &Tensor::mm(Tensor &A, Tensor &B, Tensor &O, bool inc, bool tA, bool tB) {   // Tensor::mm/gemm3 tensor.cu:73-77,161-180
    const uint32_t H = tA ? A.W() : A.H(), W = tB ? B.H() : B.W();
    const uint32_t Ka = tA ? A.H() : A.W(), Kb = tB ? B.W() : B.H();
    const uint32_t Na = A.N(), Nb = B.N(), C = B.C(), N = std::max(Na, Nb);
    if (Ka != Kb || N != O.N() || C != O.C()) { hprintf("  tensor#gemm3 ka(%d)!=kb(%d) or N, C diff\n", Ka, Kb); return O; }
    for (uint32_t n = 0; n < N; n++)
        chk(t4k_gemm(A.slice(Na == 1 ? 0 : n), B.slice(Nb == 1 ? 0 : n), O.slice(n), 1.0f, inc ? 1.0f : 0.0f, tA, tB, H, W, Ka, C, stream()), "gemm");
    return O;
}
// The batched products `@` gains beyond the reference's _tdot (tenvm.cpp:277-287 gives NumPy @ as the meaning): O[n] = A[n] @ B[n]
// for n < max(Na, Nb), an operand with N == 1 broadcast over the batch and one with C == 1 over the channels.  A is [M,K] per
// sample (a vector is [1,K]), B [K,P], O [M,P].  One t4k_gemm_batched launch; t4k_gemm_batched is referenced weakly so that the
// host sources still link over a C-ABI without it (the CPU oracle), which then takes the per-matrix t4k_gemm loop below.
#pragma weak t4k_gemm_batched
Tensor &Tensor::bmm(Tensor &A, Tensor &B, Tensor &O, uint32_t M, uint32_t K, uint32_t P) {
    const uint32_t Na = A.N(), Nb = B.N(), Ca = A.C(), Cb = B.C(), N = std::max(Na, Nb), C = std::max(Ca, Cb);
    const long sA = Na == 1 ? 0 : (long)A.HWC(), sB = Nb == 1 ? 0 : (long)B.HWC(), sO = (long)O.HWC();
    if (t4k_gemm_batched) {
        chk(t4k_gemm_batched(A.data, B.data, O.data, 1.0f, 0.0f, 0, 0, M, P, K, C, Ca, Cb, N, sA, sB, sO, stream()), "gemm_batched");
        return O;
    }
    for (uint32_t n = 0; n < N; n++) {
        const float *a = A.data + n * sA, *b = B.data + n * sB;
        float *o = O.data + n * sO;
        if (Ca == Cb)  chk(t4k_gemm(a, b, o, 1.0f, 0.0f, 0, 0, M, P, K, C, stream()), "gemm");
        else if (Ca == 1) chk(t4k_gemm(a, b, o, 1.0f, 0.0f, 0, 0, M, P * C, K, 1, stream()), "gemm");   // [M,K] @ [K,P*C]
        else for (uint32_t m = 0; m < M; m++)                                                         // row m: [P,C] = B^T @ A[m] ([K,C])
            chk(t4k_gemm(b, a + (size_t)m * K * C, o + (size_t)m * P * C, 1.0f, 0.0f, 1, 0, P, C, K, 1, stream()), "gemm");
    }
    return O;
}
Tensor &Tensor::gemm(int variant, Tensor &A, Tensor &B, Tensor &O, DU alpha, DU beta) {   // words gemm, gemm1..4 (tensor.cu:97-201)
    const uint32_t H = A.H(), W = B.W(), Ka = A.W(), Kb = B.H();
    const uint32_t Na = A.N(), Nb = B.N(), C = B.C(), N = std::max(Na, Nb);
    if (variant == 0) {                                  // word `gemm` (tensor.cu:97-123: a blocked loop on the HOST in the reference): the MFMA kernel, same alpha / beta
        chk(t4k_gemm(A.data, B.data, O.data, alpha, beta, 0, 0, H, W, Ka, 1, stream()), "gemm");
        return O;
    }
    if (Ka != Kb || N != O.N() || C != O.C()) { hprintf("  tensor#gemm%d ka(%d)!=kb(%d) or N, C diff\n", variant, Ka, Kb); return O; }
    for (uint32_t n = 0; n < N; n++) {
        float *da = A.slice(Na == 1 ? 0 : n), *db = B.slice(Nb == 1 ? 0 : n);
        if (variant <= 2) chk(t4k_gemm_f64acc(da, db, O.slice(n), alpha, beta, H, W, Ka, C, stream()), "gemm_f64acc");
        else              chk(t4k_gemm(da, db, O.slice(n), alpha, beta, 0, 0, H, W, Ka, C, stream()), "gemm");
    }
    return O;
}
Tensor &Tensor::transpose(Tensor &A, Tensor &T) {
    if (A.rank == 4 && t4k_transpose_batched) {          // a batch T4[N,H,W,C] -> T4[N,W,H,C] in one launch (beyond the reference)
        chk(t4k_transpose_batched(A.data, T.data, A.H(), A.W(), A.C(), A.N(), stream()), "transpose_batched");
        return T;
    }
    for (uint32_t n = 0; n < A.N(); n++) chk(t4k_transpose(A.slice(n), T.slice(n), A.H(), A.W(), A.C(), stream()), "transpose");
    return T;
}
// Axis permutation (beyond the reference, whose `transpose` swaps H and W of one matrix: k_transpose t4math.cu:150): T = A with output
// axis i taking A's axis perm[i] (0 = N ... 3 = C), NumPy's transpose(perm).  One t4k_permute call.  The symbol is referenced weakly: over a
// C-ABI without it (the CPU oracle) the order is reached by at most six swaps of neighbouring axes (a bubble sort of the axes by their
// place in the output), each swap one t4k_transpose(H = the outer axis, W = the inner one, C = everything inside them) per index of the
// axes outside them, ping-ponging between two temporaries and landing in T: pure copies, so the same bits.
#pragma weak t4k_permute
Tensor &Tensor::permute(Tensor &A, Tensor &T, const int perm[4]) {
    long e[4]; nhwc_of(A, e);
    if (t4k_permute) {
        const int dim[4] = { (int)e[0], (int)e[1], (int)e[2], (int)e[3] };
        chk(t4k_permute(A.data, T.data, dim, perm, stream()), "permute");
        return T;
    }
    int place[4], swaps[6], ns = 0;                      // place[k]: where the axis now at position k goes
    for (int i = 0; i < 4; i++) place[perm[i]] = i;
    for (int pass = 0; pass < 3; pass++) for (int k = 0; k < 3 - pass; k++)
        if (place[k] > place[k + 1]) { std::swap(place[k], place[k + 1]); swaps[ns++] = k; }
    if (!ns) { chk(t4k_copy(A.data, T.data, (long)A.numel, stream()), "copy"); return T; }
    Tensor *tmp[2] = { ns > 1 ? &Store::get().tensor(A.numel) : nullptr, ns > 2 ? &Store::get().tensor(A.numel) : nullptr };
    const float *src = A.data;
    for (int i = 0; i < ns; i++) {
        const int k = swaps[i];
        float *dst = i == ns - 1 ? T.data : tmp[i & 1]->data;
        long outer = 1, inner = 1;
        for (int j = 0; j < k; j++) outer *= e[j];
        for (int j = k + 2; j < 4; j++) inner *= e[j];
        const long blk = e[k] * e[k + 1] * inner;
        for (long o = 0; o < outer; o++) chk(t4k_transpose(src + o * blk, dst + o * blk, (int)e[k], (int)e[k + 1], (int)inner, stream()), "transpose");
        std::swap(e[k], e[k + 1]);
        src = dst;
    }
    for (Tensor *t : tmp) if (t) Store::get().free(*t);
    return T;
}
// Box windows (beyond the reference, whose `slice` cuts H and W with one memcpy per (sample, row): mmu.cu:307-330): the box of
// extents ext at soff of S lands at doff of D, both viewed as (N,H,W,C); nothing else of D is written.  One t4k_window call.  The
// symbol is referenced weakly: over a C-ABI without it (the CPU oracle) the box is walked run by run - the trailing axes taken whole on
// both sides and the innermost cut one are one contiguous t4k_copy - so both VMs give the same bits.  for_each_group is not the walk
// here: it gathers a group into a temporary row, and a box has two sides and nothing to gather.
void Tensor::window(Tensor &S, const int soff[4], Tensor &D, const int doff[4], const int ext[4]) {
    long es[4], ed[4]; nhwc_of(S, es); nhwc_of(D, ed);
    if (t4k_window) {
        const int sdim[4] = { (int)es[0], (int)es[1], (int)es[2], (int)es[3] }, ddim[4] = { (int)ed[0], (int)ed[1], (int)ed[2], (int)ed[3] };
        chk(t4k_window(S.data, sdim, soff, D.data, ddim, doff, ext, stream()), "window");
        return;
    }
    long ss[4], ds[4], a = 1, b = 1, run = ext[3];
    for (int i = 3; i >= 0; i--) { ss[i] = a; a *= es[i]; ds[i] = b; b *= ed[i]; }
    int top = 3;                                         // the axes from `top` inwards are one run
    while (top > 0 && ext[top] == es[top] && ext[top] == ed[top]) { top--; run *= ext[top]; }
    long k[4] = { 0, 0, 0, 0 };
    const long K[4] = { top > 0 ? ext[0] : 1, top > 1 ? ext[1] : 1, top > 2 ? ext[2] : 1, 1 };
    for (k[0] = 0; k[0] < K[0]; k[0]++) for (k[1] = 0; k[1] < K[1]; k[1]++) for (k[2] = 0; k[2] < K[2]; k[2]++) {
        long so = 0, dn = 0;
        for (int i = 0; i < 4; i++) { so += (soff[i] + k[i]) * ss[i]; dn += (doff[i] + k[i]) * ds[i]; }
        chk(t4k_copy(S.data + so, D.data + dn, run, stream()), "copy");
    }
}
static int read_status() { int s = 0; t4k_memcpy_d2h(&s, g_iscalar, sizeof(int), stream()); t4k_sync(stream()); return s; }
Tensor &Tensor::inverse(Tensor &A, Tensor &I) {          // tensor.cu:344-369
    if (A.H() != A.W() || I.H() != I.W()) { hprintf(" A: square matrix required (%d x %d)\n", A.H(), A.W()); return A; }
    const int K = A.W();
    hprintf("  tensor#inverse [%d,%d]\n", K, K);
    chk(t4k_inverse(A.data, I.data, K, g_iscalar, stream()), "inverse");
    int st = read_status();
    if (st) { hprintf("  tensor#inverse: singular matrix at column %d\n", st - 1); return A; }
    return I;
}
Tensor &Tensor::plu(Tensor &A, Tensor &I, int *piv_dev) {
    if (A.H() != A.W()) { hprintf(" A: square matrix required (%d x %d)\n", A.H(), A.W()); return A; }
    chk(t4k_plu(A.data, (&A == &I) ? nullptr : I.data, piv_dev, A.W(), g_iscalar, stream()), "plu");
    int st = read_status();
    if (st) { hprintf("  tensor#plu: singular at column %d\n", st - 1); return A; }
    return I;
}
Tensor &Tensor::lu_inverse(Tensor &A, Tensor &I) {
    if (A.H() != A.W() || I.H() != I.W()) return I;
    const int K = A.W();
    hprintf("  tensor#lu_inverse [%d,%d]\n", K, K);
    Tensor &piv = Store::get().tensor(K);
    chk(t4k_lu_inverse(A.data, I.data, (int *)piv.data, K, g_iscalar, stream()), "lu_inverse");
    int st = read_status();
    if (st) hprintf("  tensor#plu: singular at column %d\n", st - 1);
    Store::get().free(piv);
    return I;
}
Tensor &Tensor::lu(Tensor &LU, bool get_u) {
    if (LU.H() != LU.W()) return LU;
    chk(t4k_lu_extract(LU.data, get_u, LU.H(), stream()), "lu");
    return LU;
}
DU Tensor::det() {                                      // tensor.cu:431-456
    const int K = H();
    Tensor &piv = Store::get().tensor(K);
    plu(*this, *this, (int *)piv.data);
    std::vector<int> hp(K);
    t4k_memcpy_d2h(hp.data(), piv.data, sizeof(int) * K, stream()); t4k_sync(stream());
    int cnt = 0; for (int i = 0; i < K; i++) if (hp[i] != i) cnt++;
    const int sign = (cnt % 2 == 0) ? 1 : -1;
    t4k_logdet(data, K, g_scalar, g_iscalar, stream());
    DU ld = read_scalar(); int dsign = read_status();
    Store::get().free(piv);
    DU d = expf(ld) * sign * dsign;
    return SCALAR(d);
}
// The linear-algebra words over a batch T4[N,K,K,1] (beyond the reference, whose words take one rank-2 matrix: tenvm.cpp:134-216):
// entry n is treated as the rank-2 word treats its matrix.  One t4k_*_batched launch and ONE read-back of an int[N] status array per
// call; a singular entry prints the rank-2 word's line with " entry n" appended and does not stop the others.  The five symbols are
// referenced weakly: over a C-ABI without them (the CPU oracle) the same methods loop over the entries with the per-matrix calls,
// the host filling the identity those expect.
#pragma weak t4k_inverse_batched
#pragma weak t4k_plu_batched
#pragma weak t4k_lu_inverse_batched
#pragma weak t4k_lu_extract_batched
#pragma weak t4k_det_batched
static void batch_status(const int *st_dev, int N, bool gauss_jordan, std::vector<int> *keep = nullptr) {
    std::vector<int> st(N);
    t4k_memcpy_d2h(st.data(), st_dev, sizeof(int) * N, stream()); t4k_sync(stream());
    for (int n = 0; n < N; n++) {
        if (!st[n]) continue;
        if (gauss_jordan) hprintf("  tensor#inverse: singular matrix at column %d entry %d\n", st[n] - 1, n);
        else              hprintf("  tensor#plu: singular at column %d entry %d\n", st[n] - 1, n);
    }
    if (keep) keep->swap(st);
}
Tensor &Tensor::inverse_b(Tensor &A, Tensor &X, bool use_lu) {
    const int K = A.W(), N = A.N();
    if (use_lu) hprintf("  tensor#lu_inverse [%d,%d]\n", K, K); else hprintf("  tensor#inverse [%d,%d]\n", K, K);
    Tensor &ws = Store::get().tensor((uint64_t)N * (K + 1));             // int piv[N][K], status[N]
    int *piv = (int *)ws.data, *st = piv + (size_t)N * K;
    if (use_lu ? t4k_lu_inverse_batched != nullptr : t4k_inverse_batched != nullptr) {
        if (use_lu) chk(t4k_lu_inverse_batched(A.data, X.data, piv, K, N, st, stream()), "lu_inverse_batched");
        else        chk(t4k_inverse_batched(A.data, X.data, K, N, st, stream()), "inverse_batched");
    } else {
        X.identity();
        for (int n = 0; n < N; n++) {
            if (use_lu) chk(t4k_lu_inverse(A.slice(n), X.slice(n), piv + (size_t)n * K, K, st + n, stream()), "lu_inverse");
            else        chk(t4k_inverse(A.slice(n), X.slice(n), K, st + n, stream()), "inverse");
        }
    }
    batch_status(st, N, !use_lu);
    Store::get().free(ws);
    return X;
}
Tensor &Tensor::plu_b(Tensor &A, Tensor &Pm) {
    const int K = A.W(), N = A.N();
    Tensor &ws = Store::get().tensor((uint64_t)N * (K + 1));
    int *piv = (int *)ws.data, *st = piv + (size_t)N * K;
    if (t4k_plu_batched) chk(t4k_plu_batched(A.data, Pm.data, piv, K, N, st, stream()), "plu_batched");
    else {
        Pm.identity();
        for (int n = 0; n < N; n++) chk(t4k_plu(A.slice(n), Pm.slice(n), piv + (size_t)n * K, K, st + n, stream()), "plu");
    }
    batch_status(st, N, false);
    Store::get().free(ws);
    return Pm;
}
Tensor &Tensor::lu_b(Tensor &LU, bool get_u) {
    const int K = LU.W(), N = LU.N();
    if (t4k_lu_extract_batched) chk(t4k_lu_extract_batched(LU.data, get_u, K, N, stream()), "lu_batched");
    else for (int n = 0; n < N; n++) chk(t4k_lu_extract(LU.slice(n), get_u, K, stream()), "lu");
    return LU;
}
Tensor &Tensor::det_b(Tensor &A, Tensor &D) {             // per entry the formula of Tensor::det; 0 for an entry found singular
    const int K = A.W(), N = A.N();
    Tensor &ws = Store::get().tensor((uint64_t)N * (K + 3));             // int piv[N][K], status[N]; fallback: float logdet[N], int sign[N]
    int *piv = (int *)ws.data, *st = piv + (size_t)N * K;
    if (t4k_det_batched) {
        chk(t4k_det_batched(A.data, piv, K, N, D.data, st, stream()), "det_batched");
        batch_status(st, N, false);
    } else {
        float *ld = (float *)(st + N); int *sg = (int *)(ld + N);
        for (int n = 0; n < N; n++) {
            chk(t4k_plu(A.slice(n), nullptr, piv + (size_t)n * K, K, st + n, stream()), "plu");
            t4k_logdet(A.slice(n), K, ld + n, sg + n, stream());
        }
        std::vector<int> hst, hp((size_t)N * K), hs(N); std::vector<float> hl(N), d(N);
        batch_status(st, N, false, &hst);
        t4k_memcpy_d2h(hp.data(), piv, sizeof(int) * hp.size(), stream());
        t4k_memcpy_d2h(hl.data(), ld, sizeof(float) * N, stream());
        t4k_memcpy_d2h(hs.data(), sg, sizeof(int) * N, stream()); t4k_sync(stream());
        for (int n = 0; n < N; n++) {
            int cnt = 0; for (int i = 0; i < K; i++) if (hp[(size_t)n * K + i] != i) cnt++;
            d[n] = hst[n] ? 0.0f : expf(hl[n]) * ((cnt % 2 == 0) ? 1 : -1) * hs[n];
        }
        D.from_host(d.data(), N);
    }
    Store::get().free(ws);
    return D;
}

} // namespace t4
