// model.cpp - NN model: layer factory, forward / backprop orchestration, loss, optimizers.
// Restates src/nn/model.cpp:82-310, forward.cu:28-113, backprop.cu:39-140, gradient.cu:19-169,
// loss.cpp:16-136 on top of the t4k_* C-ABI.  Everything is launched asynchronously on one
// stream; the host only synchronises when a scalar (loss, hit) is read back.
#include <chrono>
#include "t4.h"
#include <algorithm>

namespace t4 {

#define NLOG(...) do { if (trace && *trace) hprintf(__VA_ARGS__); } while (0)
#define TSHOW(t, dump) hputs(fmt_show((t), (dump)))                     /* Tensor::show(dump) */
static double trace_ms() { static const auto t0 = std::chrono::steady_clock::now(); return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }   // System::clock()

Tensor &Model::T4(uint32_t n, uint32_t h, uint32_t w, uint32_t c) { return Store::get().tensor(n, h, w, c); }
Tensor &Model::VEC(uint64_t n) { return Store::get().tensor(n); }
void Model::RAND(Tensor &t, DU scale) {                 // Model::RAND model.cpp:73-78: uniform [-scale, scale)
    chk(t4k_rand(t.data, (long)t.numel, T4K_UNIFORM, -0.5f, scale * 2.0f, stream()), "rand");
}

// ---- attention, `vector{ heads causal } linear`: its own layer kind, T4K_L_ATTN, so it joins no fused group - the run, stack, head and block
// recognisers (plan_runs, stack_at, blinear, run_backward) all name the kinds they take, and none names this one.  The layer runs t4k_attention_fwd / _bwd.
// The entries are referenced weakly: over a C-ABI without them (the CPU oracle) the layer is admitted, shaped, printed, saved and loaded, and forward /
// backprop refuse it - there is no host-side fallback.
#pragma weak t4k_attention_plan
#pragma weak t4k_attention_fwd
#pragma weak t4k_attention_bwd
// C = 3 heads d with a head size the kernels take: t4k_attention_plan's rule where the C-ABI has it (16-byte path, any workspace: the step's own call decides
// those), the same rule restated where it has not
static bool attn_admits(int N, int L, int C, int heads) {
    if (heads < 1 || C % 3 || (C / 3) % heads) return false;
    const int d = C / 3 / heads;
    if (t4k_attention_plan) { int out[8]; return t4k_attention_plan(N, L, heads, d, 0, 1, 1L << 40, out) == T4K_OK; }
    return d >= 4 && d <= 128 && d % 4 == 0 && (long)N * L * C < (1L << 31);
}
static int attn_fwd(Tensor &in, Tensor &out, const float *x, t4k_stream_t s) {
    const int heads = in.iparm;
    if (!t4k_attention_fwd) { hprintf("nn#fattention failed: nn#fattention heads=%d not supported\n", heads); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_attention_fwd(x, out.data, in.grad[4]->data, in.mtum[4]->data, in.N(), in.H() * in.W(), heads, out.C() / heads, in.stride[0], s), "nn#fattention");
}
static int attn_bwd(Tensor &in, Tensor &out, const float *dy, t4k_stream_t s) {         // dX into the staging tensor, then over x: the reference's `in = dx`
    const int heads = in.iparm;
    if (!t4k_attention_bwd) { hprintf("nn#battention failed: nn#battention heads=%d not supported\n", heads); return T4K_ERR_UNSUPPORTED; }
    const int rc = chk(t4k_attention_bwd(in.data, in.grad[4]->data, dy, in.mtum[4]->data, in.mtum[0]->data, in.N(), in.H() * in.W(), heads, out.C() / heads, in.stride[0], s), "nn#battention");
    if (rc != T4K_OK) return rc;
    return chk(t4k_copy(in.mtum[0]->data, in.data, (long)in.numel, s), "nn#battention in = dx");
}
// model_load: the layer has no blobs, so its line of the layer section is all the file holds of it - `heads=<h>, causal=<0|1>` replace the layer's own where
// the channels admit them (the log-sum-exp tensor follows the head count).  false: the line is no attention line, or names heads the layer cannot have
static bool attn_from_line(Tensor &in, const std::string &line) {
    int heads = 0, causal = 0; char tail[16] = "";
    if (sscanf(line.c_str(), "heads=%d, causal=%d%15s", &heads, &causal, tail) != 3 || strcmp(tail, "attentn") || (causal != 0 && causal != 1)) return false;
    if (!attn_admits(in.N(), in.H() * in.W(), in.C(), heads)) return false;
    if (heads != in.iparm) {
        Store::get().free(*in.mtum[4]);
        in.mtum[4] = &Store::get().tensor((uint64_t)in.N() * heads * in.H() * in.W());
        in.iparm = heads;
    }
    in.stride[0] = (uint16_t)causal;
    return true;
}

// ---- add & norm, `vector{ back mode } selu`: out = norm(x + skip).  Its own layer kind, T4K_L_ADDNORM, so it joins no fused group - the run,
// stack, head and block recognisers (plan_runs, stack_at, lin_kind, blinear, run_backward) all name the kinds they take, and none names this one.  The skip
// source is the OUTPUT of an earlier layer of this kind, so this kind alone owns a skip's boundary in both directions: no other layer learns about skips.
// in.iparm = back, in.stride[0] = mode; the layer that taps this layer's output is kept in in.stride[1] | in.stride[2] << 16 (0: untapped).
// The entries are referenced weakly: over a C-ABI without them (the CPU oracle) the layer is admitted, shaped, printed, saved and loaded, and forward /
// backprop refuse it - there is no host-side fallback.
#pragma weak t4k_addnorm_plan
#pragma weak t4k_addnorm_fwd
#pragma weak t4k_addnorm_bwd
static const float ADDNORM_EPS = 1.0e-5f;
static int  an_tapper(const Tensor &in) { return (int)in.stride[1] | ((int)in.stride[2] << 16); }
static void an_set_tapper(Tensor &in, int j) { in.stride[1] = (uint16_t)(j & 0xffff); in.stride[2] = (uint16_t)(j >> 16); }
// a norm over C channels the kernels take: t4k_addnorm_plan's rule where the C-ABI has it (16-byte path - layer tensors sit on 256 bytes - and any
// workspace: the step's own call decides that), the same rule restated where it has not
static bool an_admits(long rows, int C, int mode) {
    if (t4k_addnorm_plan) { int out[8]; return t4k_addnorm_plan(rows, C, mode, 1, 1L << 40, out) == T4K_OK; }
    return rows < (1L << 31) && rows * C < (1L << 31) && (mode == 0 || C <= (C % 4 == 0 ? 8192 : 2048));
}
static int an_fwd(Tensor &in, Tensor &out, const float *x, const float *skip, t4k_stream_t s) {
    const int mode = in.stride[0];
    if (!t4k_addnorm_fwd) { hprintf("nn#faddnorm failed: nn#faddnorm mode=%d not supported\n", mode); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_addnorm_fwd(x, skip, out.data, mode ? in.grad[4]->data : nullptr, mode ? in.mtum[4]->data : nullptr, mode ? in.grad[0]->data : nullptr,
                               mode ? in.grad[1]->data : nullptr, (long)in.N() * in.H() * in.W(), in.C(), mode, ADDNORM_EPS, s), "nn#faddnorm");
}
static int an_bwd(Tensor &in, const float *dy, const float *dy2, int train, t4k_stream_t s) {      // dX = dz over x; the skip source reads the same tensor as its dy2
    const int mode = in.stride[0];
    if (!t4k_addnorm_bwd) { hprintf("nn#baddnorm failed: nn#baddnorm mode=%d not supported\n", mode); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_addnorm_bwd(mode ? in.grad[0]->data : nullptr, dy, dy2, mode ? in.grad[4]->data : nullptr, mode ? in.mtum[4]->data : nullptr, in.data,
                               mode ? in.grad[2]->data : nullptr, mode ? in.grad[3]->data : nullptr, (long)in.N() * in.H() * in.W(), in.C(), mode, train, s), "nn#baddnorm");
}
// model_load: the layer's line of the layer section must be its own, `back=<b>, mode=<m>addnorm` (the span of a skip is the model's structure, not a parameter)
static bool an_line_ok(const Tensor &in, const std::string &line) {
    int back = -1, mode = -1; char tail[16] = "";
    return sscanf(line.c_str(), "back=%d, mode=%d%15s", &back, &mode, tail) == 3 && !strcmp(tail, "addnorm") && back == in.iparm && mode == (int)in.stride[0];
}

// ---- the embedding layer, `vector{ V E pos } upsample`: a token table over the ids in the model's input, a learned position table, or both.
// Its own layer kind, T4K_L_EMBED, so it joins no fused group - the run, stack, head and block recognisers all name the kinds they take, and none names this
// one.  in.iparm = V (0: position mode), in.stride[0] = pos; grad[0] | grad[2] = TABLE T4(1, V, E, 1) and its gradient, grad[1] | grad[3] = POS T4(1, H, W, E)
// and its gradient - whichever the mode lacks stays NULL, which finalize's slab, the optimizers' table and the .t4 blobs take cell by cell (grads_ready takes
// either cell since this layer).  The entries are referenced weakly: over a C-ABI without them (the CPU oracle) the layer is admitted, shaped, printed, saved
// and loaded, and forward / backprop refuse it - there is no host-side fallback.
#pragma weak t4k_embed_plan
#pragma weak t4k_embed_fwd
#pragma weak t4k_embed_bwd
// a shape the kernels take: t4k_embed_plan's rule where the C-ABI has it (16-byte path - layer tensors sit on 256 bytes - and any workspace: the step's own
// call decides that), the same rule restated where it has not
static bool em_admits(long T, int L, int V, int E, int pos) {
    if (t4k_embed_plan) { int out[8]; return t4k_embed_plan(T, L, V, E, pos, 1, 1L << 40, out) == T4K_OK; }
    return T < (1L << 31) && T * E < (1L << 31) && (long)V * E < (1L << 31);
}
static int em_fwd(Tensor &in, Tensor &out, const float *x, t4k_stream_t s) {
    const int V = in.iparm;
    if (!t4k_embed_fwd) { hprintf("nn#fembed failed: nn#fembed vocab=%d not supported\n", V); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_embed_fwd(V ? x : nullptr, V ? nullptr : x, V ? in.grad[0]->data : nullptr, in.grad[1] ? in.grad[1]->data : nullptr, out.data,
                             (long)in.N() * in.H() * in.W(), in.H() * in.W(), V, out.C(), s), "nn#fembed");
}
static int em_bwd(Tensor &in, Tensor &out, const float *dy, int train, t4k_stream_t s) {       // position mode: dX = dY over x; token mode: the ids stay
    const int V = in.iparm;
    if (!t4k_embed_bwd) { hprintf("nn#bembed failed: nn#bembed vocab=%d not supported\n", V); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_embed_bwd(V ? in.data : nullptr, dy, in.grad[2] ? in.grad[2]->data : nullptr, in.grad[3] ? in.grad[3]->data : nullptr, V ? nullptr : in.data,
                             (long)in.N() * in.H() * in.W(), in.H() * in.W(), V, out.C(), train, s), "nn#bembed");
}
// model_load: the layer's line of the layer section must be its own, `vocab=<V>, pos=<p>embed  ` (the 7-character name; the table sizes are the model's structure)
static bool em_line_ok(const Tensor &in, const std::string &line) {
    int V = -1, pos = -1, used = 0;
    return sscanf(line.c_str(), "vocab=%d, pos=%d%n", &V, &pos, &used) == 2 && line.compare(used, std::string::npos, LAYER_NAME[T4K_L_EMBED]) == 0 &&
           V == in.iparm && pos == (int)in.stride[0];
}

// ---------------------------------------------------------------- layer factory (Model::add)
Model &Model::add(int fn, uint32_t n, DU bias, uint16_t *opt) {
    Tensor &in = at(-1);
    if (in.grad_fn != T4K_L_NONE) return *this;
    NLOG("  Model::add %s n=%d bias=%g {\n", LAYER_NAME[fn], n, bias);
    for (int i = 0; i < 5; i++) in.grad[i] = in.mtum[i] = nullptr;
    switch (fn) {
    case T4K_L_CONV: case T4K_L_DCONV: {                // _iconv model.cpp:121-180
        const bool txn = fn == T4K_L_DCONV;
        const uint32_t N1 = in.N(), H1 = in.H(), W1 = in.W(), C1 = in.C(), C0 = n;
        const uint16_t K = opt[0], S = opt[1];
        const uint16_t P = (K > 1 && opt[2]) ? opt[2] : (K - 1) / 2;
        uint16_t H0, W0, D = 0;
        uint32_t G = 1;
        if (txn) { const uint16_t P0 = (H1 + P * 2 - K) % S; H0 = (H1 - 1) * S - P * 2 + K + P0; W0 = (W1 - 1) * S - P * 2 + K + P0; }
        else {
            // conv2d takes any K 1..7 with stride, padding and dilation (the reference: "TODO: dilation" model.cpp:125): a D cell of 0 means 1
            if (K < 1 || K > 7) { hprintf("nn#iconv %s f=[%d,%d]? 1x1 to 7x7 supported only.\n", LAYER_NAME[fn], K, K); return *this; }
            D = opt[3] ? opt[3] : 1;
            if (S < 1 || S > 4 || D > 4 || P > D * (K - 1) || (int)H1 + P * 2 < D * (K - 1) + 1) {
                hprintf("nn#iconv %s stride=%d padding=%d dilation=%d?\n", LAYER_NAME[fn], S, P, D);
                return *this;
            }
            H0 = (H1 - D * (K - 1) - 1 + P * 2) / S + 1; W0 = (H1 - D * (K - 1) - 1 + P * 2) / S + 1;      // W0 from H1: reference quirk :137
            // the fifth cell cuts the channels into G groups (the reference has none): 0 or 1 = ungrouped, the filter is T4(C1 / G, K, K, C0)
            if (opt[4] > 1) {
                G = opt[4];
                if (C1 % G || C0 % G) { hprintf("nn#iconv %s groups=%d? in=%d out=%d\n", LAYER_NAME[fn], G, C1, C0); return *this; }
            }
        }
        if (txn && K != 4) {
            hprintf("nn#iconv %s f=[%d,%d]? 1x1, 3x3, 4x4, and 5x5 supported only.\n", LAYER_NAME[fn], K, K);
            return *this;
        }
        in.stride[0] = in.stride[1] = S; in.stride[2] = in.stride[3] = P; in.xparm = bias;
        in.iparm = D;                                   // convolutions use iparm for nothing else; 1 (and the 0 of a transposed layer) = undilated
        Tensor *f = in.grad[0] = &T4(C1 / G, K, K, C0);     // G is not stored: conv_G() reads it back from the filter
        Tensor *b = in.grad[1] = &VEC(C0);
        in.grad[2] = &T4(C1 / G, K, K, C0).zeros();
        in.grad[3] = &VEC(C0).zeros();
        in.grad[4] = &T4(N1, H1, W1, C1).zeros();
        RAND(*f, sqrtf(6.0f / (K * K * (C1 / G)))); RAND(*b, bias);
        layer.push_back(&T4(N1, H0, W0, C0));
    } break;
    case T4K_L_LINEAR: {                                // _ilinear model.cpp:182-226
        const uint32_t N1 = in.N(); const uint64_t E1 = in.HWC(); const uint32_t E0 = n;
        Tensor *w = in.grad[0] = &T4(1, E0, (uint32_t)E1, 1);
        Tensor *b = in.grad[1] = &VEC(E0);
        in.grad[2] = &T4(1, E0, (uint32_t)E1, 1).zeros();
        in.grad[3] = &VEC(E0).zeros();
        if (in.W() != E1) hprintf("    WARN linear: treats in[%d,%d,%d,%d] as [%d,1,%ld,1]\n", N1, in.H(), in.W(), in.C(), N1, (long)E1);
        in.xparm = bias;
        RAND(*w, sqrtf(1.0f / (E0 + E1))); RAND(*b, bias);
        layer.push_back(&T4(N1, 1, E0, 1));
    } break;
    case T4K_L_FLATTEN: layer.push_back(&T4(in.N(), 1, (uint32_t)in.HWC(), 1)); break;
    case T4K_L_RELU: case T4K_L_TANH: case T4K_L_SIGMOID: case T4K_L_SELU: case T4K_L_LEAKYRL: case T4K_L_ELU: case T4K_L_DROPOUT:
        in.grad[4] = &T4(in.N(), in.H(), in.W(), in.C()); in.xparm = bias;
        layer.push_back(&T4(in.N(), in.H(), in.W(), in.C())); break;
    case T4K_L_SOFTMAX: case T4K_L_LOGSMAX:
        in.grad[4] = &T4(1, in.H(), in.W(), in.C());
        layer.push_back(&T4(in.N(), in.H(), in.W(), in.C())); break;
    case T4K_L_AVGPOOL: case T4K_L_MAXPOOL: case T4K_L_MINPOOL: {    // _ipool model.cpp:260-274 (ceil dims)
        if (opt) {
            // the vector form takes any K 1..16 with stride and padding on a FLOOR grid, W0 from W1 (the reference has window = stride in {2, 3} only)
            const int K = opt[0], S = opt[1], P = opt[2], H1 = in.H(), W1 = in.W(), C = in.C();
            if (K < 1 || K > 16) { hprintf("nn#ipool %s k=%dx%d? 1x1 to 16x16 supported only\n", LAYER_NAME[fn], K, K); return *this; }
            if (S < 1 || S > 16 || P > K / 2 || K > H1 + 2 * P || K > W1 + 2 * P) { hprintf("nn#ipool %s stride=%d padding=%d?\n", LAYER_NAME[fn], S, P); return *this; }
            const int H0 = (H1 + 2 * P - K) / S + 1, W0 = (W1 + 2 * P - K) / S + 1;
            in.stride[0] = K; in.stride[1] = S; in.stride[2] = P; in.stride[3] = 0;
            in.iparm = 1;                               // the mark of the vector form: pooling layers use iparm for nothing else, and {3,1,1,0} is what `3 maxpool` stores
            // max / min keep the winning tap of every output element, one byte each at a pixel pitch of 4 ceil(C / 4): bytes in a float tensor
            if (fn != T4K_L_AVGPOOL) in.grad[4] = &T4(in.N(), H0, W0, (C + 3) / 4).zeros();
            layer.push_back(&T4(in.N(), H0, W0, C));
            break;
        }
        const uint16_t k = (uint16_t)n;
        if (k != 2 && k != 3) { hprintf("nn#ipool k=%dx%d? 2x2 and 3x3 supported only\n", k, k); return *this; }
        in.stride[0] = k; in.stride[1] = 1; in.stride[2] = 1; in.stride[3] = 0;
        layer.push_back(&T4(in.N(), (in.H() + k - 1) / k, (in.W() + k - 1) / k, in.C()));
    } break;
    case T4K_L_BATCHNM: {                               // _ibatchnorm model.cpp:276-292 (dW/dB zeroed here)
        const int C = in.C();
        if (opt) {
            // the vector form `vector{ G } batchnorm` is a group norm over G groups of C / G channels per sample (the reference has none):
            // G = 1 layer norm, G = C instance norm.  gamma, beta, their gradients and xhat as for batchnorm; mtum[4] holds mean | rstd | s1 | s2 per (sample, group)
            const int G = opt[0];
            if (G < 1 || C % G) { hprintf("nn#ibatchnorm groups=%d? channels=%d\n", G, C); return *this; }
            in.grad[0] = &VEC(C).map(T4K_FILL, 1.0f); in.grad[2] = &VEC(C).zeros();
            in.grad[1] = &VEC(C).zeros();             in.grad[3] = &VEC(C).zeros();
            in.grad[4] = &T4(in.N(), in.H(), in.W(), in.C());
            in.mtum[4] = &VEC((uint64_t)4 * in.N() * G).zeros();
            in.iparm = G;                               // batchnorm uses iparm for nothing: 0 stays the reference's layer, >= 1 marks this one
            in.xparm = 0;
            layer.push_back(&T4(in.N(), in.H(), in.W(), in.C()));
            break;
        }
        in.grad[0] = &VEC(C).map(T4K_FILL, 1.0f); in.grad[2] = &VEC(C).zeros();
        in.grad[1] = &VEC(C).zeros();             in.grad[3] = &VEC(C).zeros();
        in.grad[4] = &T4(in.N(), in.H(), in.W(), in.C());
        in.mtum[4] = &VEC(C * 3).zeros();
        in.xparm = bias;
        layer.push_back(&T4(in.N(), in.H(), in.W(), in.C()));
    } break;
    case T4K_L_USAMPLE: {                               // _iup model.cpp:294-310
        // any factor 1..16 and the four methods of ntypes.h:53-58 (cubic: 1..8); the reference has 2x2 and 3x3 and ignores the method
        const uint16_t k = (uint16_t)n;
        const int me = (int)bias;
        if (me < T4K_UP_NEAREST || me > T4K_UP_CUBIC) { hprintf("nn#iup method=%d?\n", me); return *this; }
        const int kmax = me == T4K_UP_CUBIC ? 8 : 16;
        if (k < 1 || k > kmax) { hprintf("nn#iup k=%dx%d? 1x1 to %dx%d supported only\n", k, k, kmax, kmax); return *this; }
        in.iparm = me;
        in.stride[0] = k; in.stride[1] = 1; in.stride[2] = 1; in.stride[3] = 1;
        layer.push_back(&T4(in.N(), in.H() * k, in.W() * k, in.C()));
    } break;
    case T4K_L_ATTN: {
        // `vector{ heads causal } linear`: multi-head attention over the H W tokens of a sample (the reference has none).  The 3E channels of a
        // token are [ Q | K | V ], head h owning channels h d .. (h + 1) d - 1 of each E.  No parameters: grad[0..3] stay NULL and the optimizer's table skips the
        // layer.  grad[4] is the copy of the output the backward reads (out.data holds dY by then), mtum[4] the log-sum-exp per (sample, head, token), mtum[0]
        // the staging tensor the backward writes dX into before it is copied over x.  Per-sample and parameter-free: dp_bn_mode and the gradient exchange
        // of a data-parallel run do not concern it.
        const int C = in.C(), heads = opt ? opt[0] : 0, causal = (opt && opt[1]) ? 1 : 0, E = C / 3;
        if (!attn_admits(in.N(), in.H() * in.W(), C, heads)) { hprintf("nn#iattention heads=%d? channels=%d\n", heads, C); return *this; }
        in.grad[4] = &T4(in.N(), in.H(), in.W(), E);
        in.mtum[4] = &VEC((uint64_t)in.N() * heads * in.H() * in.W());
        in.mtum[0] = &T4(in.N(), in.H(), in.W(), C);
        in.iparm = heads; in.stride[0] = (uint16_t)causal; in.xparm = 0;
        layer.push_back(&T4(in.N(), in.H(), in.W(), E));
    } break;
    case T4K_L_ADDNORM: {
        // `vector{ back mode } selu`: out = norm(x + skip) (the reference has none).  With this layer's input at index j the skip is the tensor
        // at j - back, which must be the output of an earlier layer of this kind (a mark `vector{ 0 0 }`, a norm or an add) that no other add taps yet.
        // mode 1 / 2: grad[0..3] = gamma (1), beta (0) and their gradients, as a group norm's - finalize, the gradient slab, grads_ready, the optimizers and a
        // data-parallel exchange see them so; grad[4] = xhat, mtum[4] = rstd per token.  mode 0: nothing but the output.  Per token: dp_bn_mode does not
        // concern it.
        const int back = opt ? opt[0] : 0, mode = opt ? opt[1] : 0, j = (int)layer.size() - 1, C = in.C();
        auto refuse = [&](const char *why) { hprintf("nn#iaddnorm back=%d mode=%d? %s\n", back, mode, why); };
        if (mode > 2) { refuse("mode 0..2"); return *this; }
        Tensor *src = nullptr;                          // the layer whose output is tapped
        if (back >= 1) {
            if (j - back < 1) { refuse("no layer there"); return *this; }
            src = &at(j - back - 1);
            if (src->grad_fn != T4K_L_ADDNORM) { char b[48]; snprintf(b, sizeof b, "layer %d is no addnorm", j - back - 1); refuse(b); return *this; }
            if (!at(j - back).same_shape(in)) { refuse("shape"); return *this; }
            if (an_tapper(*src)) { refuse("taken"); return *this; }
        }
        if (mode && !an_admits((long)in.N() * in.H() * in.W(), C, mode)) { char b[32]; snprintf(b, sizeof b, "channels=%d", C); refuse(b); return *this; }
        if (mode) {
            in.grad[0] = &VEC(C).map(T4K_FILL, 1.0f); in.grad[2] = &VEC(C).zeros();
            in.grad[1] = &VEC(C).zeros();             in.grad[3] = &VEC(C).zeros();
            in.grad[4] = &T4(in.N(), in.H(), in.W(), C);
            in.mtum[4] = &VEC((uint64_t)in.N() * in.H() * in.W());
        }
        in.iparm = back; in.stride[0] = (uint16_t)mode; in.stride[1] = in.stride[2] = in.stride[3] = 0; in.xparm = 0;
        if (src) an_set_tapper(*src, j);                // the producing layer's backward adds the gradient this layer leaves in at(j)
        layer.push_back(&T4(in.N(), in.H(), in.W(), C));
    } break;
    case T4K_L_EMBED: {
        // `vector{ V E pos } upsample` (the reference has none).  Token mode, V >= 1: the model's first layer, its input T4[N,H,W,1] the ids as
        // floats, the output T4[N,H,W,E].  Position mode, V = 0: anywhere, out = x + POS, same shape.  TABLE draws from [-1, 1), POS from [-0.02, 0.02) (the
        // ViT / GPT-2 convention).
        const int V = (int)n, E = opt ? opt[0] : 0, pos = opt ? opt[1] : 0, C = in.C();
        auto refuse = [&](const char *why) { hprintf("nn#iembed vocab=%d dim=%d pos=%d? %s\n", V, E, pos, why); };
        if (pos > 1) { refuse("pos 0..1"); return *this; }
        if (V < 0) { refuse("vocab"); return *this; }
        if (V == 0 && pos == 0) { refuse("no table"); return *this; }
        if (V >= 1 && layer.size() != 1) { refuse("not the first layer"); return *this; }
        if (V >= 1 && C != 1) { refuse("ids have 1 channel"); return *this; }
        if (V >= 1 && E < 1) { refuse("dim"); return *this; }
        if (V == 0 && E != 0 && E != C) { refuse("dim is the channels"); return *this; }
        const int E0 = V ? E : C;
        if (!em_admits((long)in.N() * in.H() * in.W(), (int)(in.H() * in.W()), V, E0, pos)) { refuse("shape"); return *this; }
        if (V) { in.grad[0] = &T4(1, V, E0, 1); in.grad[2] = &T4(1, V, E0, 1).zeros(); RAND(*in.grad[0], 1.0f); }
        if (pos) { in.grad[1] = &T4(1, in.H(), in.W(), E0); in.grad[3] = &T4(1, in.H(), in.W(), E0).zeros(); RAND(*in.grad[1], 0.02f); }
        in.iparm = V; in.stride[0] = (uint16_t)pos; in.stride[1] = in.stride[2] = in.stride[3] = 0; in.xparm = 0;
        layer.push_back(&T4(in.N(), in.H(), in.W(), E0));
    } break;
    default: hprintf("Model#add layer %d not supported\n", fn); return *this;
    }
    in.grad_fn = fn;
    invalidate();
    Tensor &out = at(-1);
    NLOG("  } Model::add[%ld] %s => out[%d,%d,%d,%d]\n", (long)layer.size(), LAYER_NAME[fn], out.N(), out.H(), out.W(), out.C());
    return *this;
}

// ---------------------------------------------------------------- execution engine
// Both are OFF by default: measured on MI355X (ROCm 7.2, LeNet step, 40 launches) the single in-order stream is the
// fastest schedule - 0.26 ms/step vs 0.28 (hipGraph replay) vs 0.31 (forked side stream; every cross-queue event edge
// costs more than the ~4.5 us in-order dispatch it hides).  What pays is fewer launches (fused kernels below).
// ---- conv2d layers outside the reference's four geometries.  ONE predicate decides the route at every call site of the conv family:
// such a layer runs t4k_conv2d_geo_fwd / _bwd and joins no fused group.  So does a GROUPED layer of any geometry, on t4k_conv2d_grp_fwd /
// _bwd: the same predicate keeps it out of every fused group, stack, conv + batch-norm epilogue and the lazy-dX0 stack path.  The entries are referenced
// weakly: over a C-ABI without them (the CPU oracle) the layer keeps the refusal at forward / backprop.
#pragma weak t4k_conv2d_geo_fwd
#pragma weak t4k_conv2d_geo_bwd
#pragma weak t4k_conv2d_grp_fwd
#pragma weak t4k_conv2d_grp_bwd
static int conv_D(const Tensor &in) { return in.iparm > 1 ? in.iparm : 1; }
static int conv_G(const Tensor &in) { return (int)(in.shape[2] / in.grad[0]->N()); }     // the filter is T4(C1 / G, K, K, C0)
static bool conv_geo(const Tensor &in) {
    if (in.grad_fn != T4K_L_CONV) return false;
    const int K = in.grad[0]->H(), S = in.stride[0], P = in.stride[2];
    const bool four = (K == 1 && S == 1 && P == 0) || (K == 3 && S == 1 && P == 1) || (K == 4 && S == 2 && P == 1) || (K == 5 && S == 1 && P == 2);
    return !four || conv_D(in) > 1 || conv_G(in) > 1;
}
static void geo_refusal(const char *who, int K, int S, int P, int D, int G) {      // the line the four-geometry entries leave through chk(), the dilation and the groups named where there are any
    char grp[24] = ""; if (G > 1) snprintf(grp, sizeof grp, " groups=%d", G);
    if (D > 1) hprintf("%s failed: %s kernel_size=%d stride=%d padding=%d dilation=%d%s not supported\n", who, who, K, S, P, D, grp);
    else       hprintf("%s failed: %s kernel_size=%d stride=%d padding=%d%s not supported\n", who, who, K, S, P, grp);
}
static int geo_fwd(Tensor &in, Tensor &out, const float *x, float *cp, t4k_stream_t s) {
    const int K = in.grad[0]->H(), S = in.stride[0], P = in.stride[2], G = conv_G(in);
    if (G > 1) {
        if (!t4k_conv2d_grp_fwd) { geo_refusal("nn#fconv", K, S, P, conv_D(in), G); return T4K_ERR_UNSUPPORTED; }
        return chk(t4k_conv2d_grp_fwd(x, cp, out.data, in.grad[0]->data, in.grad[1]->data, out.N(), in.H(), in.W(), in.C(), out.H(), out.W(), out.C(),
                                      K, S, P, conv_D(in), G, s), "nn#fconv");
    }
    if (!t4k_conv2d_geo_fwd) { geo_refusal("nn#fconv", K, S, P, conv_D(in), 1); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_conv2d_geo_fwd(x, cp, out.data, in.grad[0]->data, in.grad[1]->data, out.N(), in.H(), in.W(), in.C(), out.H(), out.W(), out.C(),
                                  K, S, P, conv_D(in), s), "nn#fconv");
}
static int geo_bwd(Tensor &in, Tensor &out, const float *dy, float *dx, float *dx2, const float *w, bool grads, int train, t4k_stream_t s) {
    const int K = in.grad[0]->H(), S = in.stride[0], P = in.stride[2], G = conv_G(in);
    if (G > 1) {
        if (!t4k_conv2d_grp_bwd) { geo_refusal("nn#bconv", K, S, P, conv_D(in), G); return T4K_ERR_UNSUPPORTED; }
        return chk(t4k_conv2d_grp_bwd(in.data, dy, dx, dx2, w, grads ? in.grad[2]->data : nullptr, grads ? in.grad[3]->data : nullptr,
                                      in.N(), in.H(), in.W(), in.C(), out.H(), out.W(), out.C(), K, S, P, conv_D(in), G, train, s), "nn#bconv");
    }
    if (!t4k_conv2d_geo_bwd) { geo_refusal("nn#bconv", K, S, P, conv_D(in), 1); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_conv2d_geo_bwd(in.data, dy, dx, dx2, w, grads ? in.grad[2]->data : nullptr, grads ? in.grad[3]->data : nullptr,
                                  in.N(), in.H(), in.W(), in.C(), out.H(), out.W(), out.C(), K, S, P, conv_D(in), train, s), "nn#bconv");
}
// ---- pooling layers of the vector form, `vector{ K S P } maxpool | avgpool | minpool`.  ONE predicate decides the route at every call site of
// the pool family: such a layer runs t4k_pool_geo_fwd / _bwd and joins no fused run, stack or block.  The entries are referenced weakly: over a C-ABI
// without them (the CPU oracle) the layer is admitted, shaped and printed, and forward / backprop refuse it - there is no host-side fallback.
#pragma weak t4k_pool_geo_fwd
#pragma weak t4k_pool_geo_bwd
static bool pool_geo(const Tensor &in) {
    return (in.grad_fn == T4K_L_AVGPOOL || in.grad_fn == T4K_L_MAXPOOL || in.grad_fn == T4K_L_MINPOOL) && in.iparm == 1;
}
static unsigned char *pool_codes(Tensor &in) { return in.grad[4] ? (unsigned char *)in.grad[4]->data : nullptr; }
static int pool_geo_fwd(Tensor &in, Tensor &out, const float *x, t4k_stream_t s) {
    const int K = in.stride[0], S = in.stride[1], P = in.stride[2];
    if (!t4k_pool_geo_fwd) { hprintf("nn#fpool failed: nn#fpool kernel_size=%d stride=%d padding=%d not supported\n", K, S, P); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_pool_geo_fwd(in.grad_fn, x, out.data, pool_codes(in), out.N(), in.H(), in.W(), in.C(), out.H(), out.W(), K, S, P, s), "nn#fpool");
}
static int pool_geo_bwd(Tensor &in, Tensor &out, const float *dy, t4k_stream_t s) {      // dX over x, the reference's in-place convention: the backward reads no forward input
    const int K = in.stride[0], S = in.stride[1], P = in.stride[2];
    if (!t4k_pool_geo_bwd) { hprintf("nn#bpool failed: nn#bpool kernel_size=%d stride=%d padding=%d not supported\n", K, S, P); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_pool_geo_bwd(in.grad_fn, pool_codes(in), dy, in.data, out.N(), in.H(), in.W(), in.C(), out.H(), out.W(), K, S, P, s), "nn#bpool");
}
// ---- upsample layers beyond the reference's form, any factor 1..16 and the methods linear / bilinear / cubic.  ONE predicate decides the
// route at both call sites: `2 upsample` and `3 upsample` with method 0 keep t4k_dpool / t4k_pool + scale, every other layer runs t4k_upsample_fwd / _bwd.
// No upsample layer joins a fused run, stack or block.  The entries are referenced weakly: over a C-ABI without them (the CPU oracle) the layer is
// admitted, shaped and printed, and forward / backprop refuse it - there is no host-side fallback.
#pragma weak t4k_upsample_fwd
#pragma weak t4k_upsample_bwd
static bool up_geo(const Tensor &in) {
    return in.grad_fn == T4K_L_USAMPLE && ((in.stride[0] != 2 && in.stride[0] != 3) || in.iparm != T4K_UP_NEAREST);
}
static int up_geo_fwd(Tensor &in, Tensor &out, const float *x, t4k_stream_t s) {
    const int K = in.stride[0];
    if (!t4k_upsample_fwd) { hprintf("nn#fupsample failed: nn#fupsample size=%d method=%d not supported\n", K, in.iparm); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_upsample_fwd(in.iparm, x, out.data, in.N(), in.H(), in.W(), in.C(), out.H(), out.W(), K, s), "nn#fupsample");
}
static int up_geo_bwd(Tensor &in, Tensor &out, const float *dy, t4k_stream_t s) {        // dX over x in ONE launch: the backward reads no forward input
    const int K = in.stride[0];
    if (!t4k_upsample_bwd) { hprintf("nn#bupsample failed: nn#bupsample size=%d method=%d not supported\n", K, in.iparm); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_upsample_bwd(in.iparm, dy, in.data, in.N(), in.H(), in.W(), in.C(), out.H(), out.W(), K, s), "nn#bupsample");
}
// ---- group / layer / instance norm, `vector{ G } batchnorm`.  ONE predicate decides the route at every reader of T4K_L_BATCHNM: such a layer runs
// t4k_groupnorm_fwd / _bwd, joins no conv + batch-norm epilogue, run, stack or block, has no running statistics and never exchanges across ranks
// (dp_bn_mode does not concern it).  The entries are referenced weakly: over a C-ABI without them (the CPU oracle) the layer is admitted, shaped and
// printed, and forward / backprop refuse it - there is no host-side fallback.
#pragma weak t4k_groupnorm_fwd
#pragma weak t4k_groupnorm_bwd
static const float NORM_GRP_EPS = 1.0e-5f;
bool norm_grp(const Tensor &in) { return in.grad_fn == T4K_L_BATCHNM && in.iparm >= 1; }
static int norm_grp_fwd(Tensor &in, Tensor &out, const float *x, t4k_stream_t s) {
    if (!t4k_groupnorm_fwd) { hprintf("nn#fbatchnorm failed: nn#fbatchnorm groups=%d not supported\n", in.iparm); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_groupnorm_fwd(x, out.data, in.grad[4]->data, in.grad[0]->data, in.grad[1]->data, in.mtum[4]->data,
                                 out.N(), out.H() * out.W(), out.C(), in.iparm, NORM_GRP_EPS, s), "nn#fbatchnorm");
}
static int norm_grp_bwd(Tensor &in, const float *dy, int train, t4k_stream_t s) {        // dX over x, as batchnorm leaves it
    if (!t4k_groupnorm_bwd) { hprintf("nn#bbatchnorm failed: nn#bbatchnorm groups=%d not supported\n", in.iparm); return T4K_ERR_UNSUPPORTED; }
    return chk(t4k_groupnorm_bwd(in.grad[0]->data, dy, in.grad[4]->data, in.mtum[4]->data, in.data, in.grad[2]->data, in.grad[3]->data,
                                 in.N(), in.H() * in.W(), in.C(), in.iparm, train, s), "nn#bbatchnorm");
}

Model *Model::current = nullptr;
void (*Model::grad_hook)(int, long, long, void *) = nullptr;
void *Model::grad_hook_user = nullptr;
bool Model::use_fusion = env_flag("T4_FUSE", true);
bool Model::use_stack  = env_flag("T4_STACK", true);
bool Model::use_head_bwd = env_flag("T4_HEAD_BWD", true);    // classifier-head backward and the linear layer in front of it in ONE launch (round 6: k_head_bwd_l32, 9.7 us; T4_HEAD_BWD=0: head on column stripes + dual GEMM, 6.9 + 5.6 us)
bool Model::use_stack_head = env_flag("T4_STACK_HEAD", true);   // T4_STACK_HEAD=0: the classifier head behind a conv stack keeps its own launches
bool Model::use_lazy_dx0 = env_flag("T4_LAZY_DX0", true);
bool Model::use_opt_fold = env_flag("T4_OPT_FOLD", true);   // T4_OPT_FOLD=0: the conv stack's partial fold keeps its own launch behind the backward
bool Model::use_graphs = env_flag("T4_GRAPH", false);
bool Model::use_side   = getenv("T4_SIDE")  ? atoi(getenv("T4_SIDE"))  != 0 : false;

// Lazy dX of the first layer.  `in = dx` (backprop.cu:185) leaves the gradient w.r.t. the input batch in layer 0 and in the first conv
// layer's scratch tensor; a training loop never reads either.  The conv-stack backward skips it (t4k_conv_stack_bwd, train | 8) and the
// two tensors carry a mark; the first word that resolves one of them (Store::du2obj: `0 n@`, `0 nn.ex`, ten4_fetch, a chained backprop ...)
// has it produced from the dO and the filter copy that backward left.  The next forward overwrites layer 0 and ends the offer (after it
// `0 nn.ex` would show an EARLIER backward's dX - the one observable difference; T4_LAZY_DX0=0 restores the eager store).
// A first LINEAR layer (an MLP: the GAN discriminator's 784 -> 512 layer is a third of its backward launch) takes the same offer: the
// backward computes dW | dB only; dX0 = dY W is produced on demand from the dY the backward left and the weights OF THAT BACKWARD - the
// weight tensor and the tensor holding dY carry the mark as well, and an optimizer step in between snapshots the old weights inside its
// own launch (t4k_opt_snapshot).
void Model::clear_dx0_marks() {
    if (!dx0_stale_) return;
    dx0_stale_ = false;
    if (!layer.empty()) { at(0).stale_owner = nullptr; if (at(0).grad[4]) at(0).grad[4]->stale_owner = nullptr; }
    if (dx0_lin_) {
        if (!layer.empty() && at(0).grad[0]) at(0).grad[0]->stale_owner = nullptr;
        if (dx0_dy_t_) dx0_dy_t_->stale_owner = nullptr;
        dx0_lin_ = false; dx0_conv_ = false; w0_saved_ = false; dx0_dy_ = nullptr; dx0_dy_t_ = nullptr;
    }
}
void Model::materialize_dx0() {
    if (!dx0_stale_) return;
    if (dx0_lin_) {
        Tensor &in = at(0), &o = at(1);
        const float *w = w0_saved_ ? w0_save_->data : in.grad[0]->data, *dy = dx0_dy_;
        const bool conv = dx0_conv_;
        clear_dx0_marks();
        if (conv && conv_geo(in)) { geo_bwd(in, o, dy, in.grad[4]->data, in.data, w, false, 0, stream()); return; }
        if (conv) {                                     // dX into the scratch tensor and over x, as the eager launch leaves them (backprop.cu:185)
            chk(t4k_conv2d_bwd2(in.data, dy, in.grad[4]->data, in.data, w, nullptr, nullptr, in.N(), in.H(), in.W(), in.C(), o.H(), o.W(), o.C(),
                                in.grad[0]->H(), in.stride[0], in.stride[2], 0, stream()), "nn#bconv dX0");
            return;
        }
        chk(t4k_linear_bwd(in.data, w, dy, in.data, nullptr, nullptr, in.N(), (int)o.HWC(), (int)in.HWC(), 0, stream()), "nn#blinear dX0");
        return;
    }
    clear_dx0_marks();
    t4k_conv_stage stg[3]; int ops = 0;
    if (stack_at(0, stg, ops) > 0) chk(t4k_conv_stack_dx0(stg, at(0).N(), stream()), "nn#bstack dX0");
}
void Model::invalidate() {
    clear_dx0_marks();
    for (GraphSlot *g : { &g_fwd_, &g_bwd_, &g_opt_ }) { if (g->g) t4k_graph_destroy(g->g); *g = GraphSlot(); }
    finalized_ = false;
}
void Model::finalize() {                                // gradient slab: SURVEY 8(e), one contiguous all-reduce buffer
    if (finalized_) return;
    finalized_ = true;
    auto pad = [](uint64_t n) { return (n + 63) & ~(uint64_t)63; };          // keep every tensor 256 B aligned
    uint64_t total = 0;
    capturable_ = true;
    for (Tensor *t : gx_) if (t) Store::get().free(*t);
    gx_.assign(layer.size(), nullptr);
    for (int i = 0; i + 1 < (int)layer.size(); i++) {
        Tensor &in = at(i);
        for (int k = 2; k < 4; k++) if (in.grad[k]) total += pad(in.grad[k]->numel);
        if (use_side && in.grad_fn == T4K_L_LINEAR && i + 2 < (int)layer.size()) gx_[i] = &T4(in.N(), in.H(), in.W(), in.C());
    }
    if (total) {
        Tensor *slab = &VEC(total).zeros();
        uint64_t off = 0;
        for (int i = 0; i + 1 < (int)layer.size(); i++) {
            Tensor &in = at(i);
            for (int k = 2; k < 4; k++) {
                Tensor *g = in.grad[k]; if (!g) continue;
                chk(t4k_copy(g->data, slab->data + off, (long)g->numel, stream()), "slab");
                if (g->owns && g->data) { t4k_sync(stream()); Arena::get().free(g->data); }
                g->data = slab->data + off; g->owns = false;
                off += pad(g->numel);
            }
        }
        if (gslab) Store::get().free(*gslab);
        gslab = slab;
        if (dp_busy_) { t4k_sync(comm_s_); dp_busy_ = false; }
        dp_done_lo_ = dp_pend_lo_ = -1; dp_mixed_ = false;     // offsets of the old slab are meaningless now
    }
    if (tab_dev) { t4k_free(tab_dev); tab_dev = nullptr; }                  // parameter table holds the old pointers
    if (use_side && !side_) chk(t4k_stream_create(&side_), "side stream");
    plan_runs();
    stack_end_.assign(layer.size(), -1);                // op index of a conv stack's last op -> its first op (the conv layer); all -1 under switches with which no step takes a stack (stacks_on)
    for (int k = 0; use_fusion && use_stack && !side_ && k + 1 < (int)layer.size(); ) {
        t4k_conv_stage stg[3]; int ops = 0;
        const int ns = at(k).grad_fn == T4K_L_CONV ? stack_at(k, stg, ops) : 0;
        if (ns >= 2 || (ns == 1 && stack_single_)) { stack_end_[k + ops - 1] = k; k += ops; } else k++;
    }
    t4k_sync(stream());
}
// Fused element-wise runs: [dropout|activation] [pool] [activation] [flatten] -> one launch each way (csrc/fused.hip).
// Only mask-multiply activations qualify (sigmoid is pass-through in the reference's backprop, backprop.cu:129-131).
static bool is_mact(int f) { return f == T4K_L_RELU || f == T4K_L_TANH || f == T4K_L_SELU || f == T4K_L_LEAKYRL || f == T4K_L_ELU; }
static bool is_pool(int f) { return f == T4K_L_AVGPOOL || f == T4K_L_MAXPOOL || f == T4K_L_MINPOOL; }
static bool is_eltwise(int f) { return is_mact(f) || f == T4K_L_SIGMOID || f == T4K_L_DROPOUT; }
void Model::plan_runs() {
    const int L = (int)layer.size() - 1;                // number of ops
    run_of_.assign(layer.size(), -1); run_at_.assign(layer.size(), -1); runs_.clear();
    if (!use_fusion) return;
    for (int i = 0; i < L; ) {
        int j = i, pre = -1, pool = -1, post = -1, flat = -1;
        if (j < L && (is_mact(at(j).grad_fn) || at(j).grad_fn == T4K_L_DROPOUT)) pre = j++;
        if (j < L && is_pool(at(j).grad_fn) && !pool_geo(at(j)) && (at(j).H() % at(j).stride[0] == 0) && (at(j).W() % at(j).stride[0] == 0)) pool = j++;
        if (j < L && (pool >= 0 || pre >= 0) &&
            (is_mact(at(j).grad_fn) || (at(j).grad_fn == T4K_L_DROPOUT && !(pre >= 0 && at(pre).grad_fn == T4K_L_DROPOUT)))) post = j++;   // activation or dropout behind
                                                                // (`leakyrelu dropout` of the GAN nets, `maxpool dropout` of the CIFAR nets): one dropout per run
        if (j < L && at(j).grad_fn == T4K_L_FLATTEN && j > i) flat = j++;
        if (j - i < 2 && !(j - i == 1 && pre >= 0 && at(pre).grad_fn == T4K_L_DROPOUT)) { i++; continue; }   // a lone dropout still fuses its mask draw
        Run r; r.first = i; r.count = j - i;
        t4k_poolblock &b = r.blk; memset(&b, 0, sizeof(b)); b.KS = 1;
        if (pre >= 0)  { b.pre_layer = at(pre).grad_fn; b.pre_alpha = at(pre).xparm; b.pre_mask = at(pre).grad[4]->data; b.pre_out = at(pre + 1).data; }
        if (pool >= 0) { b.pool_layer = at(pool).grad_fn; b.KS = at(pool).stride[0]; b.pool_out = at(pool + 1).data; }
        if (post >= 0) { b.post_layer = at(post).grad_fn; b.post_alpha = at(post).xparm; b.post_mask = at(post).grad[4]->data; b.post_out = at(post + 1).data; }
        if (flat >= 0) b.copy_out = at(flat + 1).data;
        Tensor &pin = at(pool >= 0 ? pool : i), &pout = pool >= 0 ? at(pool + 1) : pin;
        r.N = at(i).N(); r.H1 = pin.H(); r.W1 = pin.W(); r.H0 = pout.H(); r.W0 = pout.W(); r.C = pin.C();
        run_of_[i] = (int)runs_.size(); std::fill(run_at_.begin() + i, run_at_.begin() + j, run_of_[i]); runs_.push_back(r);
        i = j;
    }
}
// A run of [conv KxK stride 1 "same" + element-wise run] blocks that one workgroup per image can carry through LDS (conv_stack.hip).
// Returns the number of stages (0: layer i does not start such a stack), fills the C-ABI stage records for both directions.
int Model::stack_at(int i, t4k_conv_stage *st, int &ops) {
    const int L = (int)layer.size() - 1;
    int ns = 0, j = i, cnt[3] = {0, 0, 0};
    while (ns < 3 && j < L && at(j).grad_fn == T4K_L_CONV) {
        Tensor &in = at(j), &out = at(j + 1);
        const int K = in.grad[0]->H();
        if (in.stride[0] != 1 || in.stride[2] != K / 2 || !(K & 1) || out.H() != in.H() || out.W() != in.W() || conv_geo(in)) break;   // (a dilated layer is no stage)
        t4k_conv_stage &t = st[ns]; memset(&t, 0, sizeof(t));
        t.F = in.grad[0]->data; t.B = in.grad[1]->data; t.O = out.data;
        t.DF = in.grad[2] ? in.grad[2]->data : nullptr; t.DB = in.grad[3] ? in.grad[3]->data : nullptr;
        t.X = in.data; t.DXS = in.grad[4] ? in.grad[4]->data : nullptr;
        t.H = in.H(); t.W = in.W(); t.C1 = in.C(); t.C0 = out.C(); t.K = K;
        t.run.KS = 1;
        cnt[ns] = 1;
        if (j + 1 < L && run_of_[j + 1] >= 0) { const Run &r = runs_[run_of_[j + 1]]; t.run = r.blk; cnt[ns] += r.count; }
        j += cnt[ns]; ns++;
        if (t.run.copy_out) break;                          // a flatten closes the stack
    }
    while (ns > 0 && !t4k_conv_stack_ok(st, ns, at(i).N())) ns--;     // longest prefix the kernel can hold
    ops = 0;
    for (int s = 0; s < ns; s++) ops += cnt[s];
    return ns;
}
t4k_stream_t Model::fork() {
    if (!concurrent()) return stream();
    if (ev_.size() < 16) { ev_.resize(16, nullptr); for (auto &e : ev_) t4k_event_create(&e); }
    t4k_event_t e = ev_[ev_i_++ % ev_.size()];
    t4k_event_record(e, stream()); t4k_stream_wait_event(side_, e);
    side_dirty_ = true;
    return side_;
}
void Model::join() {
    if (!side_dirty_ || !side_) { side_dirty_ = false; return; }
    t4k_event_t e = ev_[ev_i_++ % ev_.size()];
    t4k_event_record(e, side_); t4k_stream_wait_event(stream(), e);
    side_dirty_ = false;
}
void Model::lazy_copy(const float *src, Tensor &dst) {   // bookkeeping copy, off the critical path
    if (src == dst.data) return;
    chk(t4k_copy(src, dst.data, (long)dst.numel, fork()), "copy");
}
bool Model::replay(GraphSlot &slot, const void *key, int flags, const float *p) {
    capturing_ = false;
    if (!use_graphs || !capturable_ || (trace && *trace) || t4k_comm_world() > 1 || t4k_rand_shard_world() > 1) return false;   // data parallel (a communicator, or a shard set for another transport): mask draws are keyed on the host per launch, a replay would repeat them
    const bool same = slot.key == key && slot.flags == flags && (!p || memcmp(slot.p, p, sizeof(slot.p)) == 0);
    if (same && slot.g) { chk(t4k_graph_launch(slot.g, stream()), "graph launch"); return true; }
    if (!same) {                                        // new operands: run eagerly once, capture next time
        if (slot.g) { t4k_graph_destroy(slot.g); slot.g = nullptr; }
        slot.key = key; slot.flags = flags; slot.seen = 0;
        if (p) memcpy(slot.p, p, sizeof(slot.p));
    }
    if (slot.seen++ >= 1) capturing_ = t4k_graph_begin(stream()) == T4K_OK;
    return false;
}
void Model::end_capture(GraphSlot &slot, bool capturing) {
    if (!capturing) return;
    capturing_ = false;
    if (chk(t4k_graph_end(stream(), &slot.g), "graph capture") != T4K_OK) { slot.g = nullptr; use_graphs = false; return; }
    chk(t4k_graph_launch(slot.g, stream()), "graph launch");
}

// ---------------------------------------------------------------- forward
Model &Model::forward(Tensor &input) {
    Tensor &n0 = at(0);
    if (trace && *trace) TSHOW(input, true);             // preview of the input (forward.cu:31)
    if (input.numel != n0.numel) {
        hprintf("nn#forward dataset wrong shape[%d,%d,%d,%d] != model input[%d,%d,%d,%d]\n",
               input.N(), input.H(), input.W(), input.C(), n0.N(), n0.H(), n0.W(), n0.C());
        return *this;
    }
    finalize(); current = this;
    hit_flags_pending_ = false;
    NLOG("\nModel::forward starts trace=%d {", *trace);
    const double tf0 = trace_ms();
    if (!replay(g_fwd_, input.data, (int)train, nullptr)) {
        const bool cap = capturing_;
        run_forward(input);
        end_capture(g_fwd_, cap);
    }
    if (input.type == T_DATASET && trace && *trace) traced_onehot_hit((Dataset &)input);
    else
    if (input.type == T_DATASET && !hit_flags_pending_) onehot_hit((Dataset &)input);   // labels -> one-hot rows and the hit count, one launch (or none: they rode in the conv stack's head forward)
    NLOG("\n} Model::forward %5.2f ms\n", trace_ms() - tf0);
    return *this;
}
// data parallel: batch-norm statistics span all ranks during TRAINING passes only (every rank runs those in lock step); an
// evaluation pass (`0 trainable`, possibly on one rank only) uses the rank's own statistics and issues no collective
static void dp_bn_mode(bool train) {
    static const bool want = env_flag("T4_DP_SYNC_BN", true);
    if (t4k_comm_world() > 0) t4k_comm_sync_batchnorm(train && want);
}
// the classifier head [linear + activation] + [linear + softmax] at layer j, behind a conv stack (t4k_conv_stack_head_fwd)
bool Model::fill_stack_head(int j, Tensor &input, t4k_stack_head &hd) {
    Tensor &l1 = at(j), &y1 = at(j + 1), &act = at(j + 2), &y2 = at(j + 3), &prob = at(j + 4);
    memset(&hd, 0, sizeof(hd));
    hd.W1 = l1.grad[0]->data; hd.B1 = l1.grad[1]->data; hd.Y1 = y1.data;
    hd.mid_layer = y1.grad_fn; hd.mid_alpha = y1.xparm; hd.mid_mask = y1.grad[4]->data; hd.mid_out = act.data;
    hd.W2 = act.grad[0]->data; hd.B2 = act.grad[1]->data; hd.Y2 = y2.data; hd.P = prob.data;
    hd.E1 = (int)l1.HWC(); hd.E0a = (int)y1.HWC(); hd.E0b = (int)y2.HWC();
    // a dataset batch: the one-hot rows and the hit flags of Model::onehot(Dataset&) + hit (forward.cu:57-60) ride in the same launch
    if (input.type != T_DATASET || j + 5 != (int)layer.size() || capturing_ || use_graphs) return false;
    Dataset &ds = (Dataset &)input;
    const uint32_t E = (uint32_t)prob.HWC();
    if (!ds.label || ds.batch_sz < 1 || (uint32_t)ds.batch_sz > prob.N()) return false;
    if (!hot) hot = &T4(prob.N(), 1, E, 1);
    if ((uint32_t)ds.batch_sz < prob.N()) hot->zeros();     // short last batch: the rows past it stay zero and count nothing
    if (!hit_flags_ || hit_flags_n_ < (int)prob.N()) {
        if (hit_flags_) { t4k_sync(stream()); t4k_host_free(hit_flags_); t4k_free(hit_flags_dev_); }
        void *pp; chk(t4k_host_alloc(&pp, prob.N()), "nn#hit flags"); hit_flags_ = (unsigned char *)pp; hit_flags_n_ = (int)prob.N();
        chk(t4k_malloc(&pp, prob.N()), "nn#hit flags"); hit_flags_dev_ = (unsigned char *)pp;
    }
    // where the flags go: a loop that reads `nn.hit` every batch (the reference's demos, t4_30e.4th:68-76) gets them in pinned host memory -
    // its device sync makes them readable, no copy; a loop that does not keeps them on the device, where the store does not hold the
    // kernel's end behind a PCIe round trip, and the rare `nn.hit` copies them out
    hit_flags_on_dev_ = !hit_read_;
    hit_read_ = false;
    hd.label = ds.label; hd.hot = hot->data; hd.hit_flag = hit_flags_on_dev_ ? hit_flags_dev_ : hit_flags_; hd.n_label = ds.batch_sz;
    return true;
}
void Model::run_forward(Tensor &input) {
    hit_flags_pending_ = false;
    clear_dx0_marks();                                   // this pass overwrites layer 0: a skipped dX of the previous backward is gone for good
    dp_bn_mode(train);
    const int L = (int)layer.size();
    Tensor &n0 = at(0);
    const bool fused = use_fusion && !(trace && *trace) && !concurrent();
    // layer 0 holds a COPY of the batch (forward.cu:39); a first conv layer reads the batch itself and writes the copy from its own launch
    const bool copy_in_conv = fused && L > 1 && n0.grad_fn == T4K_L_CONV && input.data != n0.data;
    // what stands behind linear layer i: 0 nothing fusable, 1 classifier head, 2 lone activation / dropout, 3 element-wise run without pool / flatten
    auto lin_kind = [&](int i) -> int {
        if (!(i + 2 < L) || at(i).grad_fn != T4K_L_LINEAR) return 0;
        const int rn = run_of_[i + 1];
        if (rn >= 0 && runs_[rn].count >= 2) return runs_[rn].masks_only() ? 3 : 0;
        if (!is_eltwise(at(i + 1).grad_fn)) return 0;
        return (at(i + 2).grad_fn == T4K_L_LINEAR && i + 4 < L && at(i + 3).grad_fn == T4K_L_SOFTMAX) ? 1 : 2;
    };
    const bool copy_in_lin = fused && input.data != n0.data && lin_kind(0) >= 2;   // a first linear layer's fold launch carries the layer-0 copy
    float *cp = (copy_in_conv || copy_in_lin) ? n0.data : nullptr;   // where op 0's own launch leaves the copy (null behind op 0)
    if (!cp) lazy_copy(input.data, n0);
    bool masks = false;
    if (concurrent())                                   // side stream: draw every dropout mask up front, in layer order
        for (int i = 0; i + 1 < L; i++)
            if (at(i).grad_fn == T4K_L_DROPOUT) {
                Tensor &m = *at(i).grad[4];
                chk(t4k_dropout_mask(m.data, (long)m.numel, fork()), "rand"); masks = true;
            }
    tl_ = trace_ms();
    stack_fresh_.assign(layer.size(), 0);                // which conv stacks this forward ran through t4k_conv_stack_fwd (their saved state is current)
    const float *x = input.data;
    for (int i = 0; i + 1 < L; i++, cp = nullptr) {
        Tensor &in = at(i), &out = at(i + 1);
        if (trace && *trace) {                          // forward.cu:44-58: time since the previous layer's line, the layer, its input's sum per sample and channel
            const double tt = trace_ms();
            hprintf("\n%6.2f:%3d> %s [%2d,%2d,%2d,%2d] \xCE\xA3/n=%6.2f p=%6.3f => out[%2d,%2d,%2d,%2d]", tt - tl_, i, LAYER_NAME[in.grad_fn],
                   in.N(), in.H(), in.W(), in.C(), in.sum() / in.N() / in.C(), in.xparm, out.N(), out.H(), out.W(), out.C());
            tl_ = tt;
        }
        if (masks && in.grad_fn == T4K_L_DROPOUT) { join(); masks = false; }
        if (fused && run_of_[i] >= 0) {                 // one launch for the whole element-wise run
            const Run &r = runs_[run_of_[i]];
            chk(t4k_poolblock_fwd(x, &r.blk, r.N, r.H1, r.W1, r.H0, r.W0, r.C, stream()), "nn#frun");
            x = at(i + r.count).data; i += r.count - 1;
            continue;
        }
        if (fused && in.grad_fn == T4K_L_LINEAR && lin_kind(i) == 3) {   // linear + an element-wise run of two (`leakyrelu dropout`): everything rides in the GEMM's fold launch
            const Run &r = runs_[run_of_[i + 1]];
            chk(t4k_linear_block_fwd(x, cp, in.grad[0]->data, in.grad[1]->data, out.data, &r.blk,
                                     out.N(), (int)out.HWC(), (int)in.HWC(), stream()), "nn#flinear+run");
            x = at(i + 1 + r.count).data; i += r.count;
            continue;
        }
        if (fused && in.grad_fn == T4K_L_LINEAR && lin_kind(i) >= 1) {   // linear + lone activation / dropout: the activation rides in the GEMM's fold launch
            Tensor &act = at(i + 2);
            if (lin_kind(i) == 1) {
                // classifier head: [linear + activation] + [linear + softmax] - the second launch folds the first GEMM's split-K slabs
                Tensor &y2 = at(i + 3), &prob = at(i + 4);
                chk(t4k_mlp_head_fwd(x, in.grad[0]->data, in.grad[1]->data, out.data, out.grad_fn, out.xparm, out.grad[4]->data, act.data,
                                     act.grad[0]->data, act.grad[1]->data, y2.data, prob.data, out.N(), (int)out.HWC(), (int)in.HWC(), (int)y2.HWC(), stream()),
                    "nn#fhead");
                x = prob.data; i += 3;
                continue;
            }
            if (cp) {                                   // the copy of the batch into layer 0 goes with the same launch
                t4k_poolblock b1; memset(&b1, 0, sizeof(b1)); b1.KS = 1;
                b1.pre_layer = out.grad_fn; b1.pre_alpha = out.xparm; b1.pre_mask = out.grad[4]->data; b1.pre_out = act.data;
                chk(t4k_linear_block_fwd(x, cp, in.grad[0]->data, in.grad[1]->data, out.data, &b1, out.N(), (int)out.HWC(), (int)in.HWC(), stream()), "nn#flinear+act");
            } else
                chk(t4k_linear_act_fwd(x, in.grad[0]->data, in.grad[1]->data, out.data, out.grad_fn, out.xparm, out.grad[4]->data, act.data,
                                       out.N(), (int)out.HWC(), (int)in.HWC(), stream()), "nn#flinear+act");
            x = act.data; i++;
            continue;
        }
        if (fused && in.grad_fn == T4K_L_LINEAR && i + 2 < L && out.grad_fn == T4K_L_SOFTMAX) {     // classifier head: linear + softmax in one launch
            Tensor &prob = at(i + 2);
            chk(t4k_linear_softmax_fwd(x, in.grad[0]->data, in.grad[1]->data, out.data, prob.data, out.N(), (int)out.HWC(), (int)in.HWC(), stream()), "nn#flinear+softmax");
            x = prob.data; i++;
            continue;
        }
        if (fused && conv_geo(in)) {                    // run-time geometry: the layer alone (with the layer-0 copy), no group; what stands behind it runs as behind any lone conv
            geo_fwd(in, out, x, cp, stream());
            x = out.data; continue;
        }
        if (fused && in.grad_fn == T4K_L_CONV) {        // a conv layer and what rides in its launch: the widest group first
            t4k_conv_stage stg[3]; int ops = 0;
            const int ns = use_stack ? stack_at(i, stg, ops) : 0;
            const int j = i + ops;                      // the layer behind the stack: a classifier head [linear + activation] + [linear + softmax]?
            const bool stack = ns >= 2 || (ns == 1 && stack_single_);
            t4k_stack_head hd;
            const bool head = stack && use_stack_head && j + 1 < L && lin_kind(j) == 1, rider = head && fill_stack_head(j, input, hd);
            const Run *r1 = (i + 2 < L && run_of_[i + 1] >= 0) ? &runs_[run_of_[i + 1]] : nullptr;       // the element-wise run behind the conv, behind conv + batch-norm
            const Run *r2 = (i + 3 < L && out.grad_fn == T4K_L_BATCHNM && !norm_grp(out) && run_of_[i + 2] >= 0) ? &runs_[run_of_[i + 2]] : nullptr;
            float *F = in.grad[0]->data, *B = in.grad[1]->data;
            const int N = out.N(), H1 = in.H(), W1 = in.W(), C1 = in.C(), H0 = out.H(), W0 = out.W(), C0 = out.C(), K = in.grad[0]->H(), S = in.stride[0], P = in.stride[2];
            int last = -1;                              // the last op the launch covers
            if (head && t4k_conv_stack_head_ok(stg, ns, N, &hd)) {     // [conv + run] x n + head, one workgroup per image, activations in LDS: the whole forward pass is ONE launch
                chk(t4k_conv_stack_head_fwd(x, cp, stg, ns, N, &hd, stream()), "nn#fstack+head");
                if (rider) { hit_flags_pending_ = true; hit_pending_ = false; }
                stack_fresh_[i] = 1; last = j + 3;
            } else if (stack) {                         // [conv + run] x n
                chk(t4k_conv_stack_fwd(x, cp, stg, ns, N, stream()), "nn#fstack");
                stack_fresh_[i] = 1; last = j - 1;
            } else if (r1 && r1->blk.pool_layer && r1->blk.KS == 2) {   // conv + the run behind it: the run rides in the conv epilogue
                chk(t4k_conv2d_block_fwd(x, cp, out.data, F, B, &r1->blk, N, H1, W1, C1, H0, W0, C0, K, S, P, stream()), "nn#fconv+run");
                last = i + r1->count;
            } else if (r2) {                            // conv + batch-norm + the run behind them: the conv output is read once (statistics from the conv's epilogue, batch-norm apply inside the run's launch)
                chk(t4k_conv2d_bn_block_fwd(x, cp, out.data, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, at(i + 2).data, out.grad[4]->data, out.grad[0]->data, out.grad[1]->data,
                                            out.mtum[4]->data, &r2->blk, r2->H0, r2->W0, stream()), "nn#fconv+batchnorm+run");
                last = i + 1 + r2->count;
            } else if (i + 2 < L && out.grad_fn == T4K_L_BATCHNM && !norm_grp(out)) {   // conv + batch-norm: the statistics ride in the conv's epilogue where its kernel carries them
                chk(t4k_conv2d_bn_fwd(x, cp, out.data, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, at(i + 2).data, out.grad[4]->data, out.grad[0]->data, out.grad[1]->data,
                                      out.mtum[4]->data, stream()), "nn#fconv+batchnorm");
                last = i + 1;
            } else if (cp) {                            // the conv alone, with the layer-0 copy
                chk(t4k_conv2d_fwd2(x, cp, out.data, F, B, N, H1, W1, C1, H0, W0, C0, K, S, P, stream()), "nn#fconv");
                last = i;
            }
            if (last >= 0) { i = last; x = at(i + 1).data; continue; }
        }
        x = fstep(in, out, x);
        if (trace && *trace && out.has_nan()) {
            hprintf("nn#forward Nan in %s\n", LAYER_NAME[in.grad_fn]);
            hprintf("in=");  TSHOW(in, true);
            hprintf("out="); TSHOW(out, true);
            err = true; break;
        }
        if (trace && *trace > 1) TSHOW(out, true);      // `2 trace`: every layer's output (forward.cu:68)
    }
    join();
}
// one layer forward: reads the activations at `x` (normally in.data), writes out.data, returns where the
// next layer finds its input (_fstep forward.cu:82-113)
const float *Model::fstep(Tensor &in, Tensor &out, const float *x) {
    const int fn = in.grad_fn;
    t4k_stream_t s = stream();
    switch (fn) {
    case T4K_L_CONV:
        if (conv_geo(in)) { geo_fwd(in, out, x, nullptr, s); break; }
        chk(t4k_conv2d_fwd(x, out.data, in.grad[0]->data, in.grad[1]->data, out.N(), in.H(), in.W(), in.C(),
                           out.H(), out.W(), out.C(), in.grad[0]->H(), in.stride[0], in.stride[2], s), "nn#fconv"); break;
    case T4K_L_DCONV:                                   // transposed convolution: the scatter form of the conv backward (forward.cu:110, see csrc/dconv.hip)
        chk(t4k_dconv2d_fwd(x, out.data, in.grad[0]->data, in.grad[1]->data, out.N(), in.H(), in.W(), in.C(),
                            out.H(), out.W(), out.C(), in.grad[0]->H(), in.stride[0], in.stride[2], s), "nn#fdconv"); break;
    case T4K_L_LINEAR:
        chk(t4k_linear_fwd(x, in.grad[0]->data, in.grad[1]->data, out.data, out.N(), (int)out.HWC(), (int)in.HWC(), s), "nn#flinear"); break;
    case T4K_L_FLATTEN: lazy_copy(x, out); return x;    // a copy in the reference (forward.cu:96); the next layer reads the source
    case T4K_L_DROPOUT:                                 // mask = fresh uniform draws (already drawn up front on the side-stream schedule)
        if (!concurrent()) chk(t4k_dropout_mask(in.grad[4]->data, (long)in.grad[4]->numel, s), "rand");
        /* fall through */
    case T4K_L_RELU: case T4K_L_TANH: case T4K_L_SIGMOID: case T4K_L_SELU: case T4K_L_LEAKYRL: case T4K_L_ELU:
        chk(t4k_activate(fn, x, out.data, in.grad[4]->data, in.xparm, (long)in.numel, s), "nn#factivate"); break;
    case T4K_L_SOFTMAX: chk(t4k_softmax(x, out.data, in.N(), (int)in.HWC(), s), "nn#fsoftmax"); break;
    case T4K_L_LOGSMAX:                                 // _flogsoftmax forward.cu:245-259 (log10 and exp(x) kept: reference bug a-16)
        chk(t4k_logsoftmax(x, out.data, out.N(), (int)out.HWC(), s), "nn#flogsoftmax"); break;
    case T4K_L_AVGPOOL: case T4K_L_MAXPOOL: case T4K_L_MINPOOL:
        if (pool_geo(in)) { pool_geo_fwd(in, out, x, s); break; }
        chk(t4k_pool(fn, x, out.data, out.N(), in.H(), in.W(), out.H(), out.W(), out.C(), in.stride[0], s), "nn#fpool"); break;
    case T4K_L_BATCHNM:
        if (norm_grp(in)) { norm_grp_fwd(in, out, x, s); break; }
        chk(t4k_batchnorm_fwd(x, out.data, in.grad[4]->data, in.grad[0]->data, in.grad[1]->data, in.mtum[4]->data,
                              out.N(), out.H() * out.W(), out.C(), s), "nn#fbatchnorm"); break;
    case T4K_L_USAMPLE:                                 // nearest: broadcast each cell to a kxk tile
        if (up_geo(in)) { up_geo_fwd(in, out, x, s); break; }
        chk(t4k_dpool(T4K_L_USAMPLE, out.data, x, in.N(), out.H(), out.W(), in.H(), in.W(), in.C(), in.stride[0], s), "nn#fupsample"); break;
    case T4K_L_ATTN: attn_fwd(in, out, x, s); break;
    case T4K_L_ADDNORM: {                               // the skip is the tensor `back` layers up: an addnorm output, which no forward launch writes after its own layer's
        const int j = (int)(std::find(layer.begin(), layer.end(), &in) - layer.begin());
        an_fwd(in, out, x, in.iparm ? at(j - in.iparm).data : nullptr, s); break;
    }
    case T4K_L_EMBED: em_fwd(in, out, x, s); break;
    default: hprintf("nn#fstep layer=%d not supported\n", fn);
    }
    return out.data;
}

// ---------------------------------------------------------------- one-hot / hit / loss
Tensor &Model::onehot() {
    if (hot) return *hot;
    hprintf("Model.onehot not provided by dataset, use nn.onehot= to setup!\n");
    return at(-1);
}
Tensor &Model::onehot(Tensor &t) {
    Tensor &out = at(-1);
    const uint32_t N = out.N(), E = (uint32_t)out.HWC();
    if (hot) { hprintf("WARN: Model.onehot exists, replaced\n"); Store::get().free(*hot); }
    else if (t.N() != N || (uint32_t)t.HWC() != E) { hprintf("Model.onehot dimension is not [%d,1,%d,1]\n", N, E); return t; }
    hot = &t; hit_ = hit(true);
    return *hot;
}
Tensor &Model::onehot(Dataset &d) {                     // loss.cpp:47-72
    Tensor &out = at(-1);
    const uint32_t E = (uint32_t)out.HWC();
    if (!hot) hot = &T4(out.N(), 1, E, 1);
    if ((uint32_t)d.batch_sz < out.N()) hot->zeros();
    chk(t4k_onehot(d.label, hot->data, d.batch_sz, E, stream()), "nn#onehot");
    return *hot;
}
void Model::onehot_hit(Dataset &d) {                    // Model::onehot(Dataset&) + hit_lazy() (forward.cu:57-60) in one launch
    Tensor &out = at(-1);
    const uint32_t E = (uint32_t)out.HWC();
    if (!d.label || d.batch_sz < 1 || (uint32_t)d.batch_sz > out.N()) { onehot(d); hit_lazy(); return; }
    if (!hot) hot = &T4(out.N(), 1, E, 1);
    if ((uint32_t)d.batch_sz < out.N()) hot->zeros();     // short last batch: the rows past it stay zero and count nothing
    if (!hit_pin) { void *p; chk(t4k_host_alloc(&p, 64), "nn#hit"); hit_pin = (int *)p; }
    chk(t4k_onehot_hit(d.label, hot->data, out.data, d.batch_sz, (int)E, hit_pin, stream()), "nn#onehot+hit");
    hit_pending_ = true;
}
void Model::traced_onehot_hit(Dataset &d) {             // the same two steps with the text `1 trace` / `2 trace` add (loss.cpp:47-107): synchronous, on host copies
    Tensor &out = at(-1);
    const uint32_t E = (uint32_t)out.HWC(), N = (uint32_t)d.batch_sz;
    onehot(d);
    std::vector<float> h, o; std::vector<uint32_t> lab(N);
    hot->to_host(h); out.to_host(o);
    if (N) { t4k_memcpy_d2h(lab.data(), d.label, sizeof(uint32_t) * N, stream()); t4k_sync(stream()); }
    NLOG("\n  Model::onehot(ds) {\n");
    if (*trace > 1)
        for (uint32_t n = 0; n < N; n++) {
            std::string l = "    n=" + std::to_string(n) + " {"; char b[16];
            for (uint32_t e = 0; e < E; e++) { snprintf(b, sizeof(b), "%2.0f%c", h[(size_t)n * E + e], e == lab[n] ? '*' : ' '); l += b; }
            hputs(l + "}\n");
        }
    NLOG("  } Model::onehot(ds)");
    NLOG("\n  Model::hit {\n");
    int cnt = 0;
    for (uint32_t n = 0; n < out.N(); n++) {
        const float *on = o.data() + (size_t)n * E, *hn = h.data() + (size_t)n * E;
        uint32_t m = 0; for (uint32_t e = 1; e < E; e++) if (on[e] > on[m]) m = e;       // first maximum
        cnt += (int)hn[m];
        if (*trace > 1) {
            std::string l = "    "; char b[24];
            for (uint32_t e = 0; e < E; e++) { snprintf(b, sizeof(b), "%4.2f%c", on[e], fabsf(hn[e] - 1.0f) < DU_EPS ? (e == m ? '#' : '*') : (e == m ? '<' : ' ')); l += b; }
            snprintf(b, sizeof(b), " n=%d cnt=%d\n", (int)n, cnt); hputs(l + b);
        }
    }
    NLOG("  } Model::hit=%d", cnt);
    hit_ = (int)dp_sum((DU)cnt); hit_pending_ = false; hit_flags_pending_ = false;
}
void Model::hit_lazy() {                                 // count on the GPU now, read it back only if somebody asks (`nn.hit`)
    if (!hot) { hit_ = 0; hit_pending_ = false; return; }
    Tensor &out = at(-1);
    if (!hit_pin) { void *p; chk(t4k_host_alloc(&p, 64), "nn#hit"); hit_pin = (int *)p; }   // device-visible host word: the kernel's store IS the read-back
    chk(t4k_hit(out.data, hot->data, out.N(), (int)out.HWC(), hit_pin, stream()), "nn#hit");
    hit_pending_ = true;
}
// data parallel: `nn.hit` and the loss words report the WHOLE batch when the library owns a communicator - one small
// all-reduce(SUM) of the rank-local value on the VM stream (hit counts are exact in fp32 below 2^24; every rank must run the word).
// Training-mode models only: after `0 trainable` the words report the rank-local value and issue NO collective, so an evaluation
// pass may run on one rank alone (the same rule dp_bn_mode applies to the batch-norm statistics).
DU Model::dp_sum(DU v) {
    if (t4k_comm_world() < 2 || !train) return v;
    if (!hit_dev) { void *p; t4k_malloc(&p, 64); hit_dev = (int *)p; }
    float *d = (float *)hit_dev + 8, r = v;               // second half of the 64-byte scratch
    t4k_memcpy_h2d(d, &r, sizeof(float), stream());
    chk(t4k_allreduce_sum(d, 1, stream()), "allreduce (scalar)");
    t4k_memcpy_d2h(&r, d, sizeof(float), stream()); t4k_sync(stream());
    return r;
}
int Model::hit(bool recalc) {                           // loss.cpp:75-107
    if (recalc) { hit_flags_pending_ = false; hit_lazy(); }
    hit_read_ = true;
    if (hit_flags_pending_) {                             // the forward left one byte per image, in pinned host memory or on the device (see forward): add them up here
        int c = 0; const int n = std::min((int)at(-1).N(), hit_flags_n_);
        std::vector<unsigned char> fl((size_t)std::max(n, 1));
        if (hit_flags_on_dev_) t4k_memcpy_d2h(fl.data(), hit_flags_dev_, (size_t)n, stream());
        t4k_sync(stream());
        if (!hit_flags_on_dev_) memcpy(fl.data(), hit_flags_, (size_t)n);
        for (int i = 0; i < n; i++) c += fl[i] ? 1 : 0;
        hit_ = (int)dp_sum((DU)c); hit_flags_pending_ = false; hit_pending_ = false;
        return hit_;
    }
    if (hit_pending_) {
        t4k_sync(stream());                                // kernel completion makes its store to the pinned word visible (no copy command)
        const int c = *(volatile int *)hit_pin;
        hit_ = (int)dp_sum((DU)c); hit_pending_ = false;
    }
    return hit_;
}
DU Model::loss(Loss op) { return hot ? loss(op, *hot) : 0.0f; }
DU Model::loss(Loss op, Tensor &tgt) {                  // loss.cpp:119-136: non-destructive (works on a copy)
    Tensor &out = at(-1);
    if (out.numel != tgt.numel) {
        hprintf("nn::loss model output shape[%d,%d,%d,%d] != tgt[%d,%d,%d,%d]\n", out.N(), out.H(), out.W(), out.C(), tgt.N(), tgt.H(), tgt.W(), tgt.C());
        return 0;
    }
    if (loss_t) *loss_t = out; else loss_t = &Store::get().copy(out);
    const DU z = loss_t->loss(op, tgt);                  // = sum over the local rows / N_local
    { static const char *opn[] = { "MSE", "BCE", "CE", "NLL" }; NLOG("  Model#loss: %s=%6.3f\n", opn[(int)op & 3], z); }
    const int world = t4k_comm_world();
    return (world < 2 || !train) ? z : SCALAR(dp_sum(z) / (DU)world);   // equal shards (the batch size is fixed by nn.model): mean of the rank means = whole-batch mean
}

// ---------------------------------------------------------------- backprop
Model &Model::broadcast(Tensor &tgt) {                  // backprop.cu:17-29: [N,1] -> [N,HWC]
    Tensor &out = at(-1);
    const uint64_t HWC = out.HWC(); const uint32_t N = out.N();
    if (!hot) hot = &T4(N, 1, (uint32_t)HWC, 1);
    if (tgt.numel < N) hot->zeros();                    // a short target fills its rows only
    chk(t4k_broadcast_rows(tgt.data, hot->data, (int)std::min<uint64_t>(N, tgt.numel), (int)HWC, stream()), "nn#broadcast");
    return *this;
}
Model &Model::backprop() {
    if (hot) return backprop(*hot);
    hprintf("nn#backprop missing onehot vector?\n");
    return *this;
}
Model &Model::backprop(Tensor &tgt) {
    Tensor &out = at(-1);
    if (out.numel != tgt.numel) {                       // _bprep backprop.cu:75-109
        hprintf("Model#bprep: Onehot wrong shape[%d,%d,%d,%d] != [%d,%d,%d,%d], numel=%ld,%ld ", tgt.N(), tgt.H(), tgt.W(), tgt.C(),
               out.N(), out.H(), out.W(), out.C(), (long)tgt.numel, (long)out.numel);
        return *this;
    }
    finalize();
    const double tb0 = trace_ms();
    if (!replay(g_bwd_, tgt.data, (int)train, nullptr)) {
        const bool cap = capturing_;
        run_backward(tgt);
        end_capture(g_bwd_, cap);
    }
    NLOG("\n} Model::backprop %5.2f ms\n", trace_ms() - tb0);
    return *this;
}
// ---- data parallel overlap.  The slab fills tail-first (last layer's dW|dB first, tests/test_gpu_embed.py pins the order).
// Ranges complete on the main stream are queued; once a bucket is full it is all-reduced on the communication stream behind
// an event, concurrently with the backward of the earlier layers.  RCCL serialises the collectives of one communicator in
// issue order whatever stream they are on, and every rank issues the same sequence (same model, same bucket size).
// Off by default: with a one-rank communicator the two cross-stream edges on the main stream (RCCL's own ordering of the final
// reduction behind the early one + the join) cost +16 us per step (0.129 -> 0.145 ms), about what hiding a 400 KB all-reduce
// can win back on 8 GPUs - to be decided with measurements on an 8-GPU box.
int  Model::dp_overlap = (int)env_long("T4_DP_OVERLAP", 0);       // 0 off, 1 on for world > 1, 2 also for a one-rank communicator (tests)
long Model::dp_bucket  = env_long("T4_DP_BUCKET", 16384);          // floats per early all-reduce (64 KiB)
void Model::grads_ready(int i, Tensor &in) {
    Tensor *lo = in.grad[2] ? in.grad[2] : in.grad[3], *hi = in.grad[3] ? in.grad[3] : in.grad[2];    // an embedding layer has one of the two, or both
    if (!(train && gslab && lo && !lo->owns)) return;
    const long off = (long)(lo->data - gslab->data);
    const long end = (long)(hi->data - gslab->data) + (long)((hi->numel + 63) & ~(uint64_t)63);
    if (grad_hook) grad_hook(i, off, end - off, grad_hook_user);
    if (!dp_overlap || dp_mixed_ || dp_pend_lo_ < 0 || t4k_comm_world() < (dp_overlap >= 2 ? 1 : 2) || concurrent() || use_graphs || capturing_) return;
    if (end != dp_pend_lo_ || off < 0 || off >= end) { dp_mixed_ = true; return; }   // not the next range down: leave the rest to `gradient`
    dp_pend_lo_ = off;
    if (dp_done_lo_ - dp_pend_lo_ >= dp_bucket) dp_flush();
}
void Model::dp_flush() {
    if (dp_done_lo_ <= dp_pend_lo_) return;
    if (!comm_s_) { chk(t4k_stream_create(&comm_s_), "comm stream"); t4k_event_create(&dp_ev_[0]); t4k_event_create(&dp_ev_[1]); }
    t4k_event_record(dp_ev_[0], stream()); t4k_stream_wait_event(comm_s_, dp_ev_[0]);            // the range is complete on the main stream
    chk(t4k_allreduce_sum(gslab->data + dp_pend_lo_, dp_done_lo_ - dp_pend_lo_, comm_s_), "allreduce (overlapped)");
    static const bool tr = env_long("T4_DP_TRACE", 0) != 0;
    if (tr) fprintf(stderr, "dp: early all-reduce of slab [%ld, %ld)\n", dp_pend_lo_, dp_done_lo_);
    dp_done_lo_ = dp_pend_lo_; dp_busy_ = true;
}
void Model::dp_begin_backward() {
    if (!gslab) return;
    const long numel = (long)gslab->numel;
    if (dp_done_lo_ >= 0 && dp_done_lo_ < numel) {
        // a second backprop before the optimizer (gradient accumulation) finds ranges that already hold the SUM over ranks:
        // turn them back into a local share (x 1/world, exact for power-of-two worlds) so the final all-reduce of the whole
        // slab gives SUM(first) + SUM(second); no more early reductions in this accumulation window
        if (dp_busy_) { t4k_event_record(dp_ev_[1], comm_s_); t4k_stream_wait_event(stream(), dp_ev_[1]); dp_busy_ = false; }
        chk(t4k_math(T4K_SCALE, gslab->data + dp_done_lo_, 1.0f / (float)t4k_comm_world(), numel - dp_done_lo_, stream()), "dp rescale");
        dp_mixed_ = true;
    }
    dp_done_lo_ = dp_pend_lo_ = numel;
}
// T4_DP_XCHG=0: the slab is all-reduced by a collective of its own (RCCL, or the exchange's generic kernel) in front of the optimizer
static const bool use_xchg = env_flag("T4_DP_XCHG", true);
void Model::dp_finish() {                                // before the update: reduce what is left, join the communication stream
    dp_in_opt_ = false;
    if (!gslab || (t4k_comm_world() <= 0 && !t4k_xchg_active())) return;
    const long numel = (long)gslab->numel;
    const long rest = (dp_done_lo_ >= 0 && dp_done_lo_ <= numel) ? dp_done_lo_ : numel;
    // one-shot peer exchange connected and nothing reduced early: the optimizer launch sums the slab over the ranks itself (t4k_opt_step_dp)
    if (use_xchg && t4k_xchg_active() && rest == numel && !dp_busy_ && !dp_mixed_ && !use_graphs) {
        dp_in_opt_ = true; dp_done_lo_ = dp_pend_lo_ = -1;
        return;
    }
    if (rest > 0) chk(t4k_allreduce_sum(gslab->data, rest, stream()), "allreduce");
    static const bool tr = env_long("T4_DP_TRACE", 0) != 0;
    if (tr) fprintf(stderr, "dp: final all-reduce of slab [0, %ld) of %ld\n", rest, numel);
    if (dp_busy_) { t4k_event_record(dp_ev_[1], comm_s_); t4k_stream_wait_event(stream(), dp_ev_[1]); dp_busy_ = false; }
    dp_done_lo_ = dp_pend_lo_ = -1; dp_mixed_ = false;
}
void Model::run_backward(Tensor &tgt) {
    if (dx0_stale_ && dx0_lin_) materialize_dx0();      // backprop twice without a forward: the layer tensors must hold what the reference's would
    dp_bn_mode(train);
    dp_begin_backward();
    Tensor &out = at(-1);
    t4k_stream_t s = stream();
    const bool fused = use_fusion && !(trace && *trace) && !concurrent();
    int skip = 0;                                       // layers already handled by the prep launch
    const float *dy0 = nullptr;                         // ... and where they left the gradient (default: the output tensor)
    const float *tg = nullptr;                          // `out -= target` still pending: the last linear layer's backward launch performs it
    NLOG("Model::bprep input(onehot) numel=%ld OK {\n", (long)tgt.numel);     // _bprep backprop.cu:84-106 (under trace nothing is fused: the loss derivative is a launch of its own)
    switch (at(-2).grad_fn) {
    case T4K_L_SIGMOID: case T4K_L_SOFTMAX: case T4K_L_LOGSMAX:
        if (fused && layer.size() > 3 && at(-3).grad_fn == T4K_L_LINEAR) { tg = tgt.data; skip = 1; break; }   // rides in the linear backward launch
        if (fused && layer.size() > 2) {                // out -= target, and the pass-through `in = out` of the last layer, in one launch
            chk(t4k_tt_op2(T4K_SUB, out.data, tgt.data, out.data, at(-2).data, (long)out.numel, s), "bprep"); skip = 1; break;
        }
        /* fall through */
    case T4K_L_LINEAR:
        chk(t4k_tt_op(T4K_SUB, out.data, tgt.data, out.data, (long)out.numel, s), "bprep"); break;
    default: {
        if (fused && is_mact(at(-2).grad_fn) && layer.size() > 2 && run_of_[(int)layer.size() - 2] < 0 && at(-2).numel == out.numel) {   // copy + the activation's mask multiply, one launch
            chk(t4k_copy_mask(tgt.data, at(-2).grad[4]->data, out.data, at(-2).data, (long)out.numel, s), "bprep+bactivate"); skip = 1; dy0 = at(-2).data; break;
        }
        chk(t4k_copy(tgt.data, out.data, (long)out.numel, s), "bprep"); break;
    }
    }
    if (trace && *trace) TSHOW(out, true);              // the loss derivative (backprop.cu:104)
    NLOG("}\n");
    NLOG("\nModel::backprop starts trace=%d train=%d {", *trace, (int)train);
    tl_ = trace_ms();
    const float *dy = dy0 ? dy0 : out.data;             // where the gradient w.r.t. the current layer's output lives
    const bool stacks = stacks_on();
    for (int i = (int)layer.size() - 2 - skip, j = skip; i >= 0; i--, j++) {
        Tensor &in = at(i), &o = at(i + 1);
        if (trace && *trace) {                          // backprop.cu:40-58
            const double tt = trace_ms();
            hprintf("\n%6.2f:%3d> %s [%2d,%2d,%2d,%2d] p=%6.3f <= out'\xCE\xA3/n=%6.2f [%2d,%2d,%2d,%2d]", tt - tl_, i, LAYER_NAME[in.grad_fn],
                   in.N(), in.H(), in.W(), in.C(), in.xparm, o.sum() / o.N() / o.C(), o.N(), o.H(), o.W(), o.C());
            tl_ = tt;
        }
        const int k0 = stacks && j > 0 ? stack_end_[i] : -1;
        if (k0 >= 0) {                                  // a sample-resident conv stack ENDS at op i: [conv + run] x n backward in ONE launch (+ the partial fold)
            t4k_conv_stage stg[3]; int ops = 0;
            const int ns = stack_at(k0, stg, ops);
            const int bflags = (train ? 1 : 0) | ((k0 < (int)stack_fresh_.size() && stack_fresh_[k0]) ? 0 : 2) | ((use_opt_fold && !grad_hook && !capturing_) ? 4 : 0) | ((use_lazy_dx0 && k0 == 0 && !capturing_ && !use_graphs) ? 8 : 0);
            // (asked first, quietly: without the forward's saved state the whole-image kernel runs, and its windows may not fit the LDS - the per-layer kernels then)
            if (ns > 0 && k0 + ops - 1 == i && t4k_conv_stack_bwd_ok(stg, ns, at(k0).N(), bflags, s) && chk(t4k_conv_stack_bwd(dy, stg, ns, at(k0).N(), bflags, s), "nn#bstack") == T4K_OK) {
                if (k0 == 0 && use_lazy_dx0 && t4k_conv_stack_dx0_pending(stg[0].O)) {
                    dx0_stale_ = true; at(0).stale_owner = this; if (at(0).grad[4]) at(0).grad[4]->stale_owner = this;
                }
                for (int k = i; k >= k0; k--) if (at(k).grad_fn == T4K_L_CONV) grads_ready(k, at(k));      // slab segments complete, last layer first
                dy = at(k0).data; j += i - k0; i = k0;
                continue;
            }
        }
        const Run *r = fused && j > 0 && run_at_[i] >= 0 ? &runs_[run_at_[i]] : nullptr;
        if (r && r->first + r->count - 1 == i) {        // a fused run ENDS at op i
            Tensor &fin = at(r->first);
            chk(t4k_poolblock_bwd(dy, fin.data, &r->blk, r->N, r->H1, r->W1, r->H0, r->W0, r->C, s), "nn#brun");
            dy = fin.data; j += i - r->first; i = r->first;
            continue;
        }
        const Back b = bstep(i, in, o, dy, j == 0, tg);
        tg = nullptr;
        grads_ready(i, in);
        if (b.also >= 0) grads_ready(b.also, at(b.also));   // a second layer's gradients came out of the same launch
        dy = b.dy; i -= b.covered; j += b.covered;      // the launch also ran the backward of `covered` ops in front (fused plans only: nothing to trace there)
        if (trace && *trace && in.has_nan()) { hprintf("nn#backprop Nan %s\n", LAYER_NAME[in.grad_fn]); TSHOW(in, false); TSHOW(o, false); err = true; break; }
        if (trace && *trace > 1) TSHOW(in, true);       // `2 trace`: every layer's dX (backprop.cu:67)
    }
    join();
}
// The first layer's dX is read by no training loop: its backward runs dF | dB (dW | dB) only when some layer tensor holds dY - that tensor, layer 0
// and the weights carry the mark, and the first word that resolves one of them has dX0 produced (materialize_dx0).  false: no holder, dX0 is stored now.
bool Model::offer_dx0(const float *dy, bool conv) {
    Tensor &in = at(0), *holder = nullptr;
    for (int k = 1; k < (int)layer.size() && !holder; k++) if (at(k).data == dy) holder = &at(k);
    if (!holder) return false;
    dx0_stale_ = true; dx0_lin_ = true; w0_saved_ = false; dx0_dy_ = dy; dx0_dy_t_ = holder;
    in.stale_owner = this; in.grad[0]->stale_owner = this; holder->stale_owner = this;
    if (conv) { dx0_conv_ = true; in.grad[4]->stale_owner = this; }
    return true;
}
// one layer backward (_bstep backprop.cu:111-140): reads dY at `dy`, leaves dX in in.data (the reference's
// in-place convention) and returns where the previous layer finds it.  Parameter gradients and the
// `in = dX` copies run on the side stream.  `tg`: backprop's `out -= target` is still pending (run_backward).
Model::Back Model::bstep(int i, Tensor &in, Tensor &out, const float *dy, bool last, const float *tg) {
    const int fn = in.grad_fn;
    t4k_stream_t s = stream();
    switch (fn) {
    case T4K_L_CONV: {
        Tensor &dx = *in.grad[4];
        const int N = in.N(), H1 = in.H(), W1 = in.W(), C1 = in.C(), H0 = out.H(), W0 = out.W(), C0 = out.C();
        const int K = in.grad[0]->H(), S = in.stride[0], P = in.stride[2];
        const bool geo = conv_geo(in);
        if (i == 0 && train && use_lazy_dx0 && use_fusion && !(trace && *trace) && !concurrent() && !capturing_ && !use_graphs && in.grad[2] && in.grad[3] &&
            offer_dx0(dy, true)) {                      // the net's first layer: dF | dB now, dX0 when a word asks
            if (geo) { geo_bwd(in, out, dy, nullptr, nullptr, in.grad[0]->data, true, 1, s); return { in.data }; }
            chk(t4k_conv2d_bwd(in.data, dy, nullptr, in.grad[0]->data, in.grad[2]->data, in.grad[3]->data,
                               N, H1, W1, C1, H0, W0, C0, K, S, P, 1, s), "nn#bconv dF");
            return { in.data };
        }
        if (geo && !concurrent()) { geo_bwd(in, out, dy, dx.data, in.data, in.grad[0]->data, train != 0, train, s); return { in.data }; }
        if (geo) {                                      // forked: dF | dB beside dX, then x = dX
            if (train) geo_bwd(in, out, dy, nullptr, nullptr, in.grad[0]->data, true, 1, fork());
            geo_bwd(in, out, dy, dx.data, nullptr, in.grad[0]->data, false, 0, s);
            lazy_copy(dx.data, in);
            return { dx.data };
        }
        if (!concurrent()) {                            // one stream: dF|dB read x first, then dX lands in the scratch tensor AND over x
            chk(t4k_conv2d_bwd2(in.data, dy, dx.data, in.data, in.grad[0]->data, train ? in.grad[2]->data : nullptr, train ? in.grad[3]->data : nullptr,
                                N, H1, W1, C1, H0, W0, C0, K, S, P, train, s), "nn#bconv");
            return { in.data };
        }
        if (train) chk(t4k_conv2d_bwd(in.data, dy, nullptr, in.grad[0]->data, in.grad[2]->data, in.grad[3]->data,
                                      N, H1, W1, C1, H0, W0, C0, K, S, P, 1, fork()), "nn#bconv dF");
        chk(t4k_conv2d_bwd(in.data, dy, dx.data, in.grad[0]->data, nullptr, nullptr, N, H1, W1, C1, H0, W0, C0, K, S, P, 0, s), "nn#bconv dX");
        lazy_copy(dx.data, in);                         // x = dX (overwrite), backprop.cu:185 - after dF has consumed x
        return { dx.data };
    }
    case T4K_L_DCONV: {                                 // backprop.cu:137: the conv forward routine gives dX; dF|dB read x first, then `in = dx`
        Tensor &dx = *in.grad[4];
        chk(t4k_dconv2d_bwd(in.data, dy, dx.data, in.grad[0]->data, train ? in.grad[2]->data : nullptr, train ? in.grad[3]->data : nullptr,
                            in.N(), in.H(), in.W(), in.C(), out.H(), out.W(), out.C(), in.grad[0]->H(), in.stride[0], in.stride[2], train, s), "nn#bdconv");
        chk(t4k_copy(dx.data, in.data, (long)in.numel, s), "nn#bdconv in = dx");
        break;
    }
    case T4K_L_LINEAR: {
        if (last) { lazy_copy(dy, in); return { dy }; }  // linear as the last layer: pass dY (backprop.cu:119-121)
        Tensor *gx = concurrent() ? gx_[i] : nullptr;
        if (!gx) return blinear(i, in, out, dy, tg);    // single stream: reference order (dW reads X, then dX overwrites it)
        const int N = in.N(), E0 = (int)out.HWC(), E1 = (int)in.HWC();
        if (train) chk(t4k_linear_bwd(in.data, in.grad[0]->data, dy, nullptr, in.grad[2]->data, in.grad[3]->data, N, E0, E1, 1, fork()), "nn#blinear dW");
        chk(t4k_linear_bwd(in.data, in.grad[0]->data, dy, gx->data, nullptr, nullptr, N, E0, E1, 0, s), "nn#blinear dX");
        lazy_copy(gx->data, in);                        // dX lands in X's buffer (backprop.cu:240) once dW has read X
        return { gx->data };
    }
    case T4K_L_FLATTEN: case T4K_L_SIGMOID: case T4K_L_SOFTMAX: case T4K_L_LOGSMAX:
        lazy_copy(dy, in); return { dy };               // pass-through (:122,129-131)
    case T4K_L_RELU: case T4K_L_TANH: case T4K_L_SELU: case T4K_L_LEAKYRL: case T4K_L_ELU: case T4K_L_DROPOUT:
        chk(t4k_tt_op(T4K_MUL, dy, in.grad[4]->data, in.data, (long)in.numel, s), "nn#bactivate"); break;
    case T4K_L_AVGPOOL: case T4K_L_MAXPOOL: case T4K_L_MINPOOL:
        if (pool_geo(in)) { pool_geo_bwd(in, out, dy, s); break; }
        chk(t4k_dpool(fn, in.data, dy, out.N(), in.H(), in.W(), out.H(), out.W(), out.C(), in.stride[0], s), "nn#bpool"); break;
    case T4K_L_BATCHNM:
        if (norm_grp(in)) { norm_grp_bwd(in, dy, train, s); break; }
        chk(t4k_batchnorm_bwd(in.grad[0]->data, dy, in.grad[4]->data, in.data, in.grad[2]->data, in.grad[3]->data,
                              in.mtum[4]->data, in.N(), in.H() * in.W(), in.C(), train, s), "nn#bbatchnorm"); break;
    case T4K_L_USAMPLE:                                 // gradient of nearest upsampling = sum over the tile = k*k * avgpool
        if (up_geo(in)) { up_geo_bwd(in, out, dy, s); break; }
        chk(t4k_pool(T4K_L_AVGPOOL, dy, in.data, in.N(), out.H(), out.W(), in.H(), in.W(), in.C(), in.stride[0], s), "nn#bupsample");
        in.map(T4K_SCALE, (DU)(in.stride[0] * in.stride[0])); break;
    case T4K_L_ATTN: attn_bwd(in, out, dy, s); break;
    case T4K_L_ADDNORM: {
        // dz = the backward of norm(x + skip) on t = dy + dy2, stored over x.  dy2 is the gradient that arrives over the skip tapping THIS layer's output: the
        // tapping layer j' (further down, so its backward ran earlier in this pass) stored its dz into ITS input tensor at(j') with a real store - an_bwd's
        // kernel, never lazy_copy - and the same dz is what the skip receives.  Nothing writes at(j') between that store and this read: a backward launch
        // writes the INPUT tensors of the layers it covers (bstep's branches, blinear's groups, a fused run's Xb / Pb / Qb / Rb, a conv stack's X and DXS),
        // its own scratch (grad[4], gx_, mtum[0]) and parameter gradients; at(j') is the input of layer j' alone, and to every launch between the two it is
        // dy, which all of them only read (the one launch that writes its dy, the `out -= target` of the last layers, runs before any addnorm's backward
        // and on at(-1) / at(-2) behind a softmax / sigmoid, never an addnorm's input).  So after backprop a tapped tensor holds the gradient that
        // arrived from the layer behind it, not the sum; the summed gradient is in the input of the layer that produced it.
        const int tap = an_tapper(in);
        an_bwd(in, dy, tap ? at(tap).data : nullptr, train, s); break;
    }
    case T4K_L_EMBED: em_bwd(in, out, dy, train, s); break;      // position mode: dX = dY over x (the reference's `in = dx`); token mode writes nothing into the ids, so a second backprop sees them
    default: hprintf("nn#bstep layer=%d not supported\n", fn);
    }
    return { in.data };
}
// Linear layer i backward on one stream, and what rides in its launch: the pending `out -= target` (tg) and the backward of the group in front of the
// layer - mask-multiply layers and, behind a conv stack or in an MLP, the linear layer in front of those.  The cases, widest group first.
Model::Back Model::blinear(int i, Tensor &in, Tensor &out, const float *dy, const float *tg) {
    t4k_stream_t s = stream();
    const int N = in.N(), E0 = (int)out.HWC(), E1 = (int)in.HWC();
    const bool fused = use_fusion && !(trace && *trace);
    float *X = in.data, *W = in.grad[0]->data, *dW = train ? in.grad[2]->data : nullptr, *dB = train ? in.grad[3]->data : nullptr, *dY = (float *)dy;
    float *out2 = tg ? at(-2).data : nullptr;           // the pass-through `in = out` of the last layer goes with `out -= target`
    auto masks_run = [&](int k, int count) { return fused && k >= 0 && run_of_[k] >= 0 && runs_[run_of_[k]].count == count && runs_[run_of_[k]].masks_only() ? &runs_[run_of_[k]] : nullptr; };
    // a lone mask-multiply layer (dropout, relu, ...) right in front of this linear layer: its backward rides along
    if (fused && i > 0 && run_of_[i - 1] >= 0 && runs_[run_of_[i - 1]].count == 1 && !runs_[run_of_[i - 1]].blk.pool_layer && runs_[run_of_[i - 1]].blk.pre_layer) {
        Tensor &prev = at(i - 1);
        // ... and when the layer in front of THAT is the linear layer behind a conv stack's flatten (the t4_30a/30e classifier), its backward
        // joins the launch too: every GEMM tile recomputes the rows of dY1 it needs (10 terms each), so nothing waits for the head (t4k_mlp_head_bwd)
        if (tg && use_head_bwd && train && i >= 3 && at(i - 2).grad_fn == T4K_L_LINEAR && stacks_on() && stack_end_[i - 3] >= 0 &&
            at(i - 2).grad[2] && at(i - 2).grad[3] && t4k_mlp_head_bwd_ok(N, (int)at(i - 2).HWC(), E1, E0)) {
            Tensor &big = at(i - 2);
            chk(t4k_mlp_head_bwd(X, W, dY, tg, out2, prev.grad[4]->data, prev.data, in.grad[2]->data, in.grad[3]->data,
                                 big.data, big.grad[0]->data, big.grad[2]->data, big.grad[3]->data, N, (int)big.HWC(), E1, E0, s), "nn#bhead+blinear");
            return { big.data, 2, i - 2 };
        }
        if (tg) chk(t4k_loss_linear_bwd(X, W, dY, tg, out2, X, prev.grad[4]->data, prev.data, dW, dB, N, E0, E1, train, s), "nn#bprep+blinear+act");
        else    chk(t4k_linear_bwd2(X, W, dy, X, prev.grad[4]->data, prev.data, dW, dB, N, E0, E1, train, s), "nn#blinear+act");
        return { prev.data, 1 };
    }
    // a lone activation that multiplies by its derivative mask (relu, tanh, leakyrelu, ... - not a fused run, not the
    // pass-through sigmoid) in front of a layer too large for the head kernel: the multiply rides in the dX epilogue
    if (fused && i > 0 && !tg && run_at_[i - 1] < 0 && is_mact(at(i - 1).grad_fn)) {
        Tensor &prev = at(i - 1);
        t4k_poolblock b1; memset(&b1, 0, sizeof(b1)); b1.KS = 1;
        b1.pre_layer = prev.grad_fn; b1.pre_alpha = prev.xparm; b1.pre_mask = prev.grad[4]->data; b1.pre_out = X;
        chk(t4k_linear_block_bwd(X, W, dY, nullptr, nullptr, X, &b1, prev.data, dW, dB, N, E0, E1, train, s), "nn#blinear+act");
        return { prev.data, 1 };
    }
    // a run of two mask-multiply layers (`leakyrelu dropout`) in front: its backward rides along as well
    if (const Run *r = masks_run(i - 2, 2)) {
        // the linear layer in front of that run joins the launch when it is the net's first layer or has such a run of its own in front (the GAN
        // discriminator: linear, leakyrelu, dropout, linear, leakyrelu, dropout, linear, sigmoid) - t4k_mlp_block_bwd, see t4k_mlp_head_bwd
        // (measured on the GAN nets, N = 256, 256-wide runs: 28.5 us against 9 + 11.7 us apart - re-reading two 256 KB masks per tile costs more than
        // reading the finished dY1; opt-in with T4_HEAD_BWD=2)
        static const bool runs_too = env_long("T4_HEAD_BWD", 1) >= 2;
        if (tg && use_head_bwd && runs_too && i >= 3 && at(i - 3).grad_fn == T4K_L_LINEAR && (!train || (at(i - 3).grad[2] && at(i - 3).grad[3]))) {
            Tensor &big = at(i - 3);
            const Run *r1 = masks_run(i - 5, 2);
            if ((r1 || i == 3) && t4k_mlp_head_bwd_ok(N, (int)big.HWC(), E1, E0)) {
                chk(t4k_mlp_block_bwd(X, W, dY, tg, out2, &r->blk, at(i - 2).data, dW, dB,
                                      big.data, big.grad[0]->data, r1 ? &r1->blk : nullptr, r1 ? at(i - 5).data : nullptr,
                                      train ? big.grad[2]->data : nullptr, train ? big.grad[3]->data : nullptr, N, (int)big.HWC(), E1, E0, train, s), "nn#bhead+run+blinear");
                return { r1 ? at(i - 5).data : big.data, r1 ? 5 : 3, i - 3 };
            }
        }
        chk(t4k_linear_block_bwd(X, W, dY, tg, out2, X, &r->blk, at(i - 2).data, dW, dB, N, E0, E1, train, s), "nn#blinear+run");
        return { at(i - 2).data, 2 };
    }
    if (tg) chk(t4k_loss_linear_bwd(X, W, dY, tg, out2, X, nullptr, nullptr, in.grad[2]->data, in.grad[3]->data, N, E0, E1, train, s), "nn#bprep+blinear");
    else if (i == 0 && train && use_lazy_dx0 && fused && !capturing_ && !use_graphs && in.grad[2] && in.grad[3] && (long)E0 * E1 >= 16384 && offer_dx0(dy, false))
        chk(t4k_linear_bwd(X, W, dy, nullptr, in.grad[2]->data, in.grad[3]->data, N, E0, E1, 1, s), "nn#blinear dW");   // the net's first layer: dW | dB now, dX0 = dY W when a word asks
    else chk(t4k_linear_bwd(X, W, dy, X, in.grad[2]->data, in.grad[3]->data, N, E0, E1, train, s), "nn#blinear");
    return { X };
}

// ---------------------------------------------------------------- optimizers
void Model::build_table(Optim op) {                      // one multi-tensor launch replaces 6-8 launch+sync pairs
    std::vector<t4k_param_rec> recs;
    tab_max = 0; tab_chunks = 0;
    for (int i = 0; i + 1 < (int)layer.size(); i++) {
        Tensor &in = at(i);
        for (int k = 0; k < 2; k++) {
            if (!in.mtum[k] || !in.grad[k] || !in.grad[k + 2]) continue;
            t4k_param_rec r;
            r.G = in.grad[k]->data; r.DG = in.grad[k + 2]->data; r.M = in.mtum[k]->data;
            r.V = in.mtum[k + 2] ? in.mtum[k + 2]->data : in.mtum[k]->data;
            r.n = (long)in.grad[k]->numel; r.Nw = (int)in.grad[k]->N(); r.pad = tab_chunks;     // g.N(): C1 for conv filters (quirk a-19); pad = first 1024-element chunk
            tab_chunks += (int)((r.n + 1023) / 1024);
            recs.push_back(r); tab_max = std::max(tab_max, r.n);
        }
    }
    if (tab_dev) t4k_free(tab_dev);
    tab_n = (int)recs.size(); tab_kind = op; tab_dev = nullptr; tab_host_ = recs;
    if (tab_n) {
        t4k_malloc(&tab_dev, recs.size() * sizeof(t4k_param_rec));
        t4k_memcpy_h2d(tab_dev, recs.data(), recs.size() * sizeof(t4k_param_rec), stream()); t4k_sync(stream());
    }
}
Model &Model::gradient(const char *nm, Optim op, DU lr, DU b1, DU b2, DU wd) {   // gradient.cu:63-126
    NLOG("\nModel::%s starts (%s) batch_sz=%d, lr=%7.4f, mtum/b1=%6.3f, b2=%6.3f {\n", nm, train ? "trainning" : "testing", at(1).N(), lr, b1, b2);
    finalize();
    const bool first = (iter++ == 0 && epoch == 0);
    if (first || tab_kind != op) {                      // grad_alloc gradient.cu:19-59 (+ re-allocation when the optimizer is switched mid-run,
        if (first) NLOG("  #grad_alloc {\n");
        for (int i = 0; i + 1 < (int)layer.size(); i++) {   //   where the reference would read the SGD alias / a null V)
            Tensor &in = at(i); Tensor *w = in.grad[0], *b = in.grad[1];
            if (first) NLOG("    %3d> %8s w,b[%d,%d] mtum=<pool offsets>\n", i, LAYER_NAME[in.grad_fn], w ? 1 : 0, b ? 1 : 0);   // (the reference prints its pool offsets of m / v here)
            Tensor *g[2] = { w, b };
            for (int k = 0; k < 2; k++) {
                if (!g[k]) continue;
                if (op == OPTI_SGD) { if (!in.mtum[k]) in.mtum[k] = g[k]; continue; }
                if (!in.mtum[k] || in.mtum[k] == g[k]) in.mtum[k] = &T4(g[k]->N(), g[k]->H(), g[k]->W(), g[k]->C()).zeros();
                if (op != OPTI_SGDM && !in.mtum[k + 2]) in.mtum[k + 2] = &T4(g[k]->N(), g[k]->H(), g[k]->W(), g[k]->C()).zeros();
            }
        }
        if (first) NLOG("  } #grad_alloc\n");
        build_table(op);
    }
    if (!train) return *this;
    if (!tab_dev || tab_kind != op) build_table(op);
    // trace levels (gradient.cu:66-79,95-99): per layer, per parameter tensor the sums of the parameter and of its gradient before the update and the
    // parameter's sum after it; `2 trace`: small tensors (< 256 elements) dumped before and after.  The update itself is ONE launch over all tensors
    // here, so the "before" halves are collected first and the text is assembled behind the launch (the tensors are independent: same numbers).
    struct TrLine { int layer; char k; Tensor *g, *dg; std::string head, before; };
    std::vector<TrLine> trl;
    const double tg0 = trace_ms();
    if (trace && *trace)
        for (int i = 0; i + 1 < (int)layer.size(); i++) {
            Tensor &in = at(i);
            for (int k = 0; k < 2; k++) {
                if (!in.mtum[k] || !in.grad[k] || !in.grad[k + 2]) continue;
                Tensor &g = *in.grad[k], &dg = *in.grad[k + 2];
                char b[160]; const char c = k ? 'b' : 'w';
                snprintf(b, sizeof(b), "     %c[%2d,%2d,%2d,%2d] \xCE\xA3=%6.3f - %6.3f", c, g.N(), g.H(), g.W(), g.C(), g.sum(), dg.sum());
                TrLine t{ i, c, &g, &dg, b, "" };
                if (*trace > 1 && g.numel < 256) t.before = std::string("\nbefore ") + c + " =" + fmt_dump(g) + "\nbefore d" + c + "=" + fmt_dump(dg);
                trl.push_back(t);
            }
        }
    const int kind = (op == OPTI_ADAM) ? 1 : (op == OPTI_ADAMW ? 2 : 0);
    const float p[4] = { lr, b1, b2, wd };
    // data parallel: every rank holds a shard of the batch; SUM the gradient slab (raw batch sums, quirk a-19) in-order
    // on the VM stream right before the update, so N ranks x batch B reproduce one rank x batch N*B
    dp_finish();
    if (dx0_stale_ && dx0_lin_ && !w0_saved_) {          // a deferred dX0 = dY W needs the weights of its backward: the update launch leaves them in w0_save_
        Tensor &w0 = *at(0).grad[0];
        if (!w0_save_) w0_save_ = &T4(w0.N(), w0.H(), w0.W(), w0.C());
        // the snapshot rides in THIS model's next t4k_opt_step launch; an update served by a graph replay (arguments baked at capture) would never take it:
        // there the copy is a launch of its own (the request is a process-global one-shot)
        if (use_graphs || capturing_) chk(t4k_memcpy_d2d(w0_save_->data, w0.data, sizeof(float) * w0.numel, stream()), "nn#w0 copy");
        else t4k_opt_snapshot(w0.data, w0_save_->data);
        w0_saved_ = true;
    }
    if (!replay(g_opt_, tab_dev, (int)op, p)) {
        const bool cap = capturing_;
        if (dp_in_opt_) chk(t4k_opt_step_dp(kind, (const t4k_param_rec *)tab_dev, tab_host_.data(), tab_n, tab_chunks, lr, b1, b2, wd, gslab->data, (long)gslab->numel, stream()), nm);
        else chk(t4k_opt_step(kind, (const t4k_param_rec *)tab_dev, tab_host_.data(), tab_n, tab_chunks, lr, b1, b2, wd, stream()), nm);   // one workgroup per 1024 parameters (+ a conv stack's deferred partial fold)
        dp_in_opt_ = false;
        end_capture(g_opt_, cap);
    }
    if (t4k_opt_snapshot_pending()) {                    // must not happen (the launch above consumes it); never leave the request for another model's update
        t4k_opt_snapshot(nullptr, nullptr); w0_saved_ = false;
        hprintf("nn#%s: weight snapshot not taken - the first layer's deferred dX is no longer available\n", nm);
    }
    if (trace && *trace) {
        size_t q = 0;
        for (int i = 0; i + 1 < (int)layer.size(); i++) {
            hprintf("  %d> %s\n", i, LAYER_NAME[at(i).grad_fn]);
            for (; q < trl.size() && trl[q].layer == i; q++) {
                const TrLine &t = trl[q];
                hputs(t.head);
                if (!t.before.empty()) hputs(t.before + "\nafter  " + t.k + " =" + fmt_dump(*t.g) + "\nafter  d" + t.k + "=" + fmt_dump(*t.dg) + "\n");
                hprintf(" => %c\xCE\xA3=%6.3f\n", t.k, t.g->sum());
            }
        }
    }
    NLOG("} Model::%s %5.2f ms\n", nm, trace_ms() - tg0);
    return *this;
}
Model &Model::sgd(DU lr, DU b) { return gradient("sgd", ZEQ(b) ? OPTI_SGD : OPTI_SGDM, lr, iter ? b : 0.0f, 0, 0); }   // `_iter ? b : 0` gradient.cu:139
Model &Model::adam(DU lr, DU b1, DU b2) { return gradient("adam", OPTI_ADAM, lr, b1, b2, 0); }
Model &Model::adamw(DU lr, DU wd, DU b1, DU b2) { return gradient("adamw", OPTI_ADAMW, lr, b1, b2, wd); }

// ---------------------------------------------------------------- persistence (.t4 model file, aio_model.cpp)
// Layout written by the reference: a `\\ tensorForth v4.0 model` line, one `<params><layer name>` line per layer, a blank
// line, then for every conv / linear (w, b), batchnorm (w) and group-norm (w, b: `vector{ G } batchnorm`) tensor a `--- w.<layer>` marker line followed by the raw
// fp32 values, and a closing `---`.  Loading into an already built model skips the layer section and reads the blobs in
// layer order (the reference's own reload of the layer section is unfinished: `_parm` text is not Forth source).  An attention layer has
// no blob: its `heads=<h>, causal=<c>attentn` line is read back into the model's attention layer at that place.  An add & norm layer saves
// gamma and beta where it has them (mode != 0); its `back=<b>, mode=<m>addnorm` line must be the layer's own - a file with another is refused whole.  An
// embedding layer saves TABLE ('w') and POS ('b'), whichever it has; its `vocab=<V>, pos=<p>embed  ` line is held to the same.
int model_save(Model &m, const char *fname) {
    FILE *f = fopen(fname, "wb");
    if (!f) { hprintf("} => failed to open for output\n"); return 1; }
    fprintf(f, "\\ tensorForth v4.0 model\n");
    const int L = (int)m.layer.size();
    for (int i = 0; i + 1 < L; i++) { Tensor &in = m.at(i), &out = m.at(i + 1); fprintf(f, "%s%s\n", fmt_parm(in, out).c_str(), LAYER_NAME[in.grad_fn]); }
    std::vector<float> h;
    auto dump = [&](char pn, const char *nm, Tensor &t) {
        fprintf(f, "\n--- %c.%s\n", pn, nm);
        t.to_host(h); fwrite(h.data(), sizeof(float), t.numel, f);
    };
    for (int i = 0; i + 1 < L; i++) {
        Tensor &in = m.at(i); const int fn = in.grad_fn;
        if ((fn == T4K_L_CONV || fn == T4K_L_LINEAR || fn == T4K_L_DCONV) && in.grad[0] && in.grad[1]) { dump('w', LAYER_NAME[fn], *in.grad[0]); dump('b', LAYER_NAME[fn], *in.grad[1]); }   // (the reference skips dconv2d blobs, aio_model.cpp:170: a net it cannot run)
        else if (fn == T4K_L_BATCHNM && in.grad[0]) { dump('w', LAYER_NAME[fn], *in.grad[0]); if (norm_grp(in)) dump('b', LAYER_NAME[fn], *in.grad[1]); }   // batchnorm proper saves gamma alone, as the reference does
        else if (fn == T4K_L_ADDNORM && in.grad[0]) { dump('w', LAYER_NAME[fn], *in.grad[0]); dump('b', LAYER_NAME[fn], *in.grad[1]); }
        else if (fn == T4K_L_EMBED) { if (in.grad[0]) dump('w', LAYER_NAME[fn], *in.grad[0]); if (in.grad[1]) dump('b', LAYER_NAME[fn], *in.grad[1]); }   // TABLE | POS, whichever the mode has
    }
    fprintf(f, "\n---\n");
    fclose(f);
    return 0;
}
int model_load(Model &m, const char *fname) {
    FILE *f = fopen(fname, "rb");
    if (!f) { hprintf("} => failed to open for input\n"); return 1; }
    auto getline_ = [&](std::string &line) { line.clear(); int c; bool any = false; while ((c = fgetc(f)) != EOF) { any = true; if (c == '\n') break; line.push_back((char)c); } return any; };
    std::string line;
    if (m.layer.size() <= 1) {                           // nothing to load into.  The reference copies the file's layer section + " nn.load <file>" into the
        fclose(f); return 2;                             // input buffer (aio_model.cpp:183-204), which System::readline clears before any VM reads it (sys.cpp:101-108;
    }                                                    // `nn.load` is no word either): nothing is printed, nothing is loaded - observed on the reference's own VM
    std::vector<float> h;
    int err = 0;
    // the layer section is skipped (model already built), but for an add & norm layer, whose line must be the layer's own (checked first: a refused file
    // changes nothing), and an attention layer: it has no blobs, its line is rebuilt into the layer (attn_from_line)
    std::vector<std::string> lines;
    while (getline_(line) && line.length()) lines.push_back(line);
    auto line_of = [&](int i) -> const std::string & { static const std::string none; return i + 1 < (int)lines.size() ? lines[i + 1] : none; };   // (lines[0] is the header)
    for (int i = 0; i + 1 < (int)m.layer.size(); i++)
        if (m.at(i).grad_fn == T4K_L_ADDNORM && !an_line_ok(m.at(i), line_of(i))) { hprintf(" model format error (addnorm layer %d: %s)\n", i, line_of(i).c_str()); err = 1; }
    for (int i = 0; i + 1 < (int)m.layer.size() && !err; i++)                                  // ... and an embedding layer's; one error line a file
        if (m.at(i).grad_fn == T4K_L_EMBED && !em_line_ok(m.at(i), line_of(i))) { hprintf(" model format error (embed layer %d: %s)\n", i, line_of(i).c_str()); err = 1; }
    if (err) { fclose(f); return err; }
    for (int i = 0; i + 1 < (int)m.layer.size() && i + 1 < (int)lines.size(); i++) {
        if (m.at(i).grad_fn != T4K_L_ATTN) continue;
        if (!attn_from_line(m.at(i), lines[i + 1])) { hprintf(" model format error (attention layer %d: %s)\n", i, lines[i + 1].c_str()); err = 1; }
    }
    if (err) { fclose(f); return err; }
    auto rd = [&](Tensor &t) {
        while (getline_(line) && !line.length()) {}      // skip blank lines
        if (line.size() < 3 || line[0] != '-' || line[1] != '-' || line[2] != '-') { hprintf(" model format error"); err = 1; return; }   // aio_model.cpp:211 (no newline there either)
        h.resize(t.numel);
        if (fread(h.data(), sizeof(float), t.numel, f) != t.numel) { hprintf(" model format error"); err = 1; return; }
        t.from_host(h.data(), t.numel);
    };
    const int L = (int)m.layer.size();
    for (int i = 0; i + 1 < L && !err; i++) {
        Tensor &in = m.at(i); const int fn = in.grad_fn;
        if ((fn == T4K_L_CONV || fn == T4K_L_LINEAR || fn == T4K_L_DCONV) && in.grad[0] && in.grad[1]) { rd(*in.grad[0]); if (!err) rd(*in.grad[1]); }
        else if (fn == T4K_L_BATCHNM && in.grad[0]) { rd(*in.grad[0]); if (!err && norm_grp(in)) rd(*in.grad[1]); }
        else if (fn == T4K_L_ADDNORM && in.grad[0]) { rd(*in.grad[0]); if (!err) rd(*in.grad[1]); }
        else if (fn == T4K_L_EMBED) { if (in.grad[0]) rd(*in.grad[0]); if (!err && in.grad[1]) rd(*in.grad[1]); }
    }
    if (!err) {                                          // the blob list must end here: a closing `---` line and nothing else
        while (getline_(line) && !line.length()) {}
        if (line != "---") { hprintf(" model format error (layers of the file and of the model differ)\n"); err = 1; }
    }
    fclose(f);
    return err;
}

void Model::free_all() {
    invalidate();
    if (current == this) current = nullptr;
    t4k_sync(stream());
    if (side_) { t4k_stream_destroy(side_); side_ = nullptr; }
    if (comm_s_) { t4k_stream_destroy(comm_s_); comm_s_ = nullptr; for (auto &e : dp_ev_) if (e) { t4k_event_destroy(e); e = nullptr; } }
    for (auto e : ev_) if (e) t4k_event_destroy(e);
    ev_.clear();
    for (Tensor *t : gx_) if (t) Store::get().free(*t);
    gx_.clear();
    if (gslab) { Store::get().free(*gslab); gslab = nullptr; }
    if (w0_save_) { Store::get().free(*w0_save_); w0_save_ = nullptr; }
    for (int i = 0; i + 1 < (int)layer.size(); i++) if (at(i).grad_fn == T4K_L_CONV) t4k_conv_stack_release(at(i + 1).data);   // what a stack forward saved for its banded backward
    for (int i = (int)layer.size() - 1; i >= 0; i--) Store::get().free(*layer[i]);
    layer.clear();
    if (hot) { Store::get().free(*hot); hot = nullptr; }
    if (loss_t) { Store::get().free(*loss_t); loss_t = nullptr; }
    if (tab_dev) { t4k_free(tab_dev); tab_dev = nullptr; }
    if (hit_dev) { t4k_free(hit_dev); hit_dev = nullptr; }
    if (hit_pin) { t4k_sync(stream()); t4k_host_free(hit_pin); hit_pin = nullptr; }
    if (hit_flags_) { t4k_sync(stream()); t4k_host_free(hit_flags_); t4k_free(hit_flags_dev_); hit_flags_ = hit_flags_dev_ = nullptr; hit_flags_n_ = 0; }
}

Model &Store::model(int *trace) { Model *m = new Model(); m->type = T_MODEL; m->trace = trace; put(m); return *m; }
Dataset &Store::dataset(uint32_t batch) {
    Dataset *d = new Dataset(); d->type = T_DATASET; d->rank = 4; d->shape[3] = batch; d->owns = false; d->data = nullptr;
    put(d); return *d;
}

} // namespace t4
