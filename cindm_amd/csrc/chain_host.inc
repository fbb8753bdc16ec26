// The chain driver: what every sampling entry (cindm_ddpm1d_sample*, cindm_ddpm2d_sample*) does around its own step.
// Textually included by cindm_hip.hip after the 1-D U-Net's host code and before ddpm1d_host.inc and the 2-D host files; each piece
// exists once.
//   RecSpec, DesignTables, Known2D, Known1D, Multistep, Armed, cindm_ddpm1d, KeyBuilder   the schedule handle both sides run on, with what a
//                       chain call arms on it
//   chain_stream        which stream a chain runs on
//   stream_steps        the eager loop
//   graph_capture/_run  capture a step functor into an instantiated graph; launch it n times and synchronise
//   replay_once         the 2-D chains' replay: stream_steps, or capture + run + destroy (no cache)
//   upload_ddim_tables  schedule check + the DDIM loops' per-step device tables
//   ChainArmed          everything armed on the handle -- the recorder, the three table objectives' tables, the 2-D and the 1-D known
//                       region, the multistep solver -- taken by every chain entry, 1-D or 2-D, as its first statement; the entry
//                       states what of it it serves (refuse_all_but) and refuses the rest
//   rec_*               the chain recorder: run by every entry but the rollout and the Langevin chain
//   design_*            the table objectives (waypoint, quadratic, pair-distance): run by the two guided 1-D entries
//   Known2D / Known1D   the known regions: run by the four 2-D entries / by cindm_ddpm1d_sample / _sample_guided / _sample_ddim /
//                       _sample_ddim_guided
//   ms_*                the second-order multistep solver: run by cindm_ddpm1d_sample_ddim / _sample_ddim_guided and
//                       cindm_ddpm2d_sample_ddim / _sample_ddim_force (bottom of this file)
// On top of these, the 1-D entries (ddpm1d_host.inc, timecompose_host.inc) state their own facts once in Chain1D (the workspace layout), step1_refuse /
// chain1_refuse / guided_refuse, chain_io, ddim_tables1, loop_chain and guided_chain, and the four 2-D entries (ddpm2d_host.inc)
// theirs in Chain2D (the workspace layout), chain2_refuse / force_refuse, ForceGuide, ddim_args2, ddpm_step2 / ddim_step2 and run_chain2.
// The 1-D replay (replay_steps in ddpm1d_host.inc: graph cached in the handle by key, ping-pong pair + odd tail, flag polls) is built
// on the same two graph functions.

// A recorder as armed by the caller (buf .. streams) and as one chain runs it (the rest, filled by rec_begin)
struct RecSpec {
    float* buf = nullptr; int64_t buf_floats = 0; int every = 0, streams = 0;
    int n = 0; int64_t fpr = 0; float* x0_stage = nullptr;
    bool on() const { return buf != nullptr; }
};

// The device tables of a table objective as armed by the caller (cindm_ddpm1d_set_design_tables / _quadratic / _pairdist, below).
// kind: an index into kDesignKinds; (a, b) are (target, scale), (S, h) or (band, weight); width counts what that kind's facts say.
enum { kWaypoint = 0, kQuadratic = 1, kPairDist = 2, kNumDesignKinds = 3 };
struct DesignTables {
    int kind = 0; const float* a = nullptr; const float* b = nullptr; int a_per_design = 0, b_per_design = 0;
    int rows = 0, width = 0; int64_t batch = 0;
    bool taken = false;      // set by design_begin: the running chain reads these tables
    bool on() const { return a != nullptr; }
};

// The known region of a 2-D chain as armed by the caller (cindm_ddpm1d_set_known2d, below: known .. cp) and as one chain runs it
// (the rest, filled by the entry: known2_begin in ddpm2d_host.inc)
struct Known2D {
    const float* known = nullptr; const unsigned char* mask = nullptr;
    const float* zi_state = nullptr; const float* zi_bound = nullptr; const float* z_state = nullptr; const float* z_bound = nullptr;
    int64_t zs_stride = 0, zb_stride = 0, images = 0; int hw = 0, cp = 0;
    const int* tnext = nullptr; uint64_t seed = 0; int64_t sample_off = 0;
    bool on() const { return known != nullptr; }
};

// The known region of a 1-D chain as armed by the caller (cindm_ddpm1d_set_known1d, below) and checked against the chain's state by
// the entry (known1_begin in ddpm1d_host.inc)
struct Known1D {
    const float* known = nullptr; const unsigned char* mask = nullptr; int known_per_design = 0, mask_per_design = 0;
    const float* z_init = nullptr; const float* z_step = nullptr; const float* z_recur = nullptr;
    int64_t step_stride = 0, recur_stride = 0, batch = 0; int rows = 0, feats = 0, apply_init = 1;
    bool on() const { return known != nullptr; }
};

// The second-order multistep solver as armed by the caller (cindm_ddpm1d_set_multistep, bottom of this file): the per-step kappa
// (a host copy: the entry puts it beside its DDIM tables) and the caller's history buffer, shaped like the chain's state
struct Multistep {
    std::vector<float> kappa; float* hist = nullptr; int64_t hist_floats = 0;
    bool on() const { return hist != nullptr; }
};

// Everything a caller can arm on the handle for the next chain call (one slot per kind of table objective: two kinds can be armed
// at once, and a guided entry says which one does not fit).  ChainArmed, below, is how a chain entry takes it.
struct Armed {
    RecSpec rec; DesignTables tables[kNumDesignKinds]; Known2D kn; Known1D kn1; Multistep ms;
};

struct cindm_ddpm1d {
    int T = 0;
    float* tab = nullptr;        // 13 tables, each [T]
    int* t_dev = nullptr;        // device step state used by the sample loops: [0] = t, [1] = block counter, [2] = DDIM step index
    hipStream_t own = nullptr;   // capture stream used when the caller passes the legacy default stream
    // the instantiated graph of the last captured step and everything it embeds (handles + their pack generation,
    // descriptor, tensor / workspace pointers, batch): a loop with the same key replays it without a new capture
    std::vector<unsigned char> gkey; hipGraph_t graph = nullptr; hipGraphExec_t gexec = nullptr;
    int last_step_launches = 0, last_step_fused = 0;     // what the last emitted reverse step consisted of (cindm_ddpm1d_last_step_info)
    int last_chain_recovered = 0, last_chain_crowded = 0, last_chain_in_flight = 0, last_chain_range = 0;     // cindm_ddpm1d_last_chain_info
    hipGraph_t graph1 = nullptr; hipGraphExec_t gexec1 = nullptr;      // ping-pong loops: the one-step graph that ends an odd count
    Armed armed;                        // what the next chain call will take (the cindm_ddpm1d_set_* entries write it)
    int rec_info[4] = {0, 0, 0, 0};     // what the last chain recorded (cindm_ddpm1d_recorder_info)
    // what the running chain holds of what it took (null: none): its recorder, the tables of its objective (the bundle's slots, one per
    // kind: the chain runs with those design_begin marked `taken` -- one kind under descriptor modes 3 - 6, every armed kind under
    // mode 7), its known region (2-D,
    // 1-D), its multistep solver.  They point into the entry's ChainArmed, which clears them when the entry returns.
    const RecSpec* rec = nullptr; const DesignTables* dzt = nullptr; const Known2D* kn = nullptr; const Known1D* kn1 = nullptr;
    const Multistep* ms = nullptr;
    void drop_graph() {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        if (gexec1) (void)hipGraphExecDestroy(gexec1);
        if (graph1) (void)hipGraphDestroy(graph1);
        gexec = nullptr; graph = nullptr; gexec1 = nullptr; graph1 = nullptr; gkey.clear();
    }
};

struct KeyBuilder {
    std::vector<unsigned char> k;
    template <typename T> KeyBuilder& operator()(const T& v) { const auto* p = reinterpret_cast<const unsigned char*>(&v); k.insert(k.end(), p, p + sizeof(T)); return *this; }
};

// The legacy default stream cannot be captured: a graph chain handed that stream orders against it with a device synchronise
// and runs on the handle's private stream (the graph path synchronises at the end anyway).
static int chain_stream(cindm_ddpm1d* h, void* stream_, int use_graph, hipStream_t* stream) {
    *stream = (hipStream_t)stream_;
    if (use_graph && *stream == nullptr) {
        if (!h->own) HIPCHK(hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
        HIPCHK(hipDeviceSynchronize());
        *stream = h->own;
    }
    return 0;
}

// enqueue step(parity) nsteps times on the stream `step` launches to; nothing is synchronised
template <typename StepFn>
static int stream_steps(int nsteps, StepFn step) {
    for (int i = 0; i < nsteps; ++i) if (step(i & 1) != 0) return -1;
    HIPCHK(hipGetLastError());
    return 0;
}

// capture step(0) .. step(nst - 1) on `stream` into *graph and instantiate it as *exec; on failure both stay null
template <typename StepFn>
static int graph_capture(hipStream_t stream, int nst, StepFn step, hipGraph_t* graph, hipGraphExec_t* exec) {
    *graph = nullptr; *exec = nullptr;
    HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    for (int q = 0; q < nst && rc == 0; ++q) rc = step(q);
    hipError_t ce = hipStreamEndCapture(stream, graph);
    if (rc != 0) { if (*graph) (void)hipGraphDestroy(*graph); *graph = nullptr; return -1; }
    if (ce != hipSuccess) { *graph = nullptr; return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce)); }
    hipError_t ie = hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) {
        (void)hipGraphDestroy(*graph); *graph = nullptr; *exec = nullptr;
        return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
    }
    return 0;
}

// launch `exec` n times, then `tail` once (when given), then synchronise the stream
static int graph_run(hipStream_t stream, hipGraphExec_t exec, int n, hipGraphExec_t tail = nullptr) {
    hipError_t le = hipSuccess;
    for (int i = 0; i < n && le == hipSuccess; ++i) le = hipGraphLaunch(exec, stream);
    if (tail && le == hipSuccess) le = hipGraphLaunch(tail, stream);
    hipError_t se = hipStreamSynchronize(stream);
    if (le != hipSuccess) return fail(std::string("hipGraphLaunch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(std::string("hipStreamSynchronize: ") + hipGetErrorString(se));
    return 0;
}

// the 2-D chains' replay: step(parity, ignored by them) enqueues one step; with use_graph it is captured once per call and the graph launched nsteps
// times (synchronised); without, the steps are only enqueued (the caller, or cindm_forceunet_status, synchronises later)
template <typename StepFn>
static int replay_once(hipStream_t stream, int nsteps, int use_graph, StepFn step) {
    if (!use_graph) return stream_steps(nsteps, step);
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    if (graph_capture(stream, 1, step, &graph, &exec) != 0) return -1;
    const int rc = graph_run(stream, exec, nsteps);
    (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph);
    return rc;
}

// The DDIM loops' schedule (times[0 .. n_steps], strictly decreasing inside [0, T), the last may be -1) and their per-step device
// tables: [n_steps][4] floats (3 coefficients + the step's guidance weight, 0 without `weights`) at dst, then [n_steps] next-times
// (*tn_out).  dst holds n_steps * 5 words: the caller checks that (and whatever else bounds n_steps for it) before the call.
static int upload_ddim_tables(int T, int32_t n_steps, const int32_t* times, const float* coefs, float* dst, hipStream_t stream,
                              int** tn_out, const float* weights = nullptr) {
    REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    for (int i = 0; i < n_steps; ++i) REQUIRE(times[i] >= 0 && times[i] < T && times[i + 1] < times[i] && times[i + 1] >= -1, "bad DDIM time schedule");
    std::vector<float> tabv((size_t)n_steps * 4, 0.f);
    std::vector<int> tnv(n_steps);
    for (int i = 0; i < n_steps; ++i) {
        tabv[4 * i] = coefs[3 * i]; tabv[4 * i + 1] = coefs[3 * i + 1]; tabv[4 * i + 2] = coefs[3 * i + 2];
        if (weights) tabv[4 * i + 3] = weights[i];
        tnv[i] = times[i + 1];
    }
    int* tn_dev = reinterpret_cast<int*>(dst + (size_t)n_steps * 4);
    HIPCHK(hipMemcpyAsync(dst, tabv.data(), tabv.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(tn_dev, tnv.data(), tnv.size() * sizeof(int), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));            // the host vectors go out of scope
    *tn_out = tn_dev;
    return 0;
}

// ---- what a chain call takes (the rule of everything armed) ---------------------------------------------------------------------------
// The cindm_ddpm1d_set_* entries arm the handle.  The next chain entry, 1-D or 2-D, takes ALL of it with a ChainArmed as its first
// statement -- so the call consumes what was armed however it ends -- and then either runs with a thing or refuses it with the
// reason: refuse_all_but names what the entry serves, and the served things are checked against the chain by their *_begin
// (rec_begin, design_begin, known1_begin, known2_begin, ms_begin), which hand them to the handle's running-chain pointers for the
// whole call, the recovery re-run included.  The destructor clears those pointers.  (The recorder is taken by every entry; the two
// that do not record refuse it themselves, with their own reason.)
enum : unsigned { kServesTables = 1, kServesKnown2 = 2, kServesKnown1 = 4, kServesMultistep = 8 };

struct ChainArmed : Armed {
    cindm_ddpm1d* h;
    explicit ChainArmed(cindm_ddpm1d* h_) : h(h_) {
        if (!h) return;
        static_cast<Armed&>(*this) = std::move(h->armed); h->armed = Armed();
        for (int& v : h->rec_info) v = 0;
    }
    ~ChainArmed() { if (h) { h->rec = nullptr; h->dzt = nullptr; h->kn = nullptr; h->kn1 = nullptr; h->ms = nullptr; } }
    ChainArmed(const ChainArmed&) = delete;
    ChainArmed& operator=(const ChainArmed&) = delete;
    // the refusal of the first armed thing that `serves` does not name, in one order for every entry: waypoint, quadratic and
    // pair-distance tables, 2-D known region, 1-D known region (why_known1: the entry's reason), multistep solver
    int refuse_all_but(unsigned serves, const char* why_known1 = nullptr) const;
};

// ---- the chain recorder (DESIGN 4.5l) --------------------------------------------------------------------------------------------------
// cindm_ddpm1d_set_recorder arms the handle; a chain entry either refuses the recorder it took or runs with it:
//   rec_begin   checks it against the chain (steps, floats per record) before the entry's first launch or copy
//   rec_arm     writes the device descriptor; part of what a chain body does after it has set the step state, so a re-run re-arms
//   rec_node    the step's chain_record_kernel launch (captured with the step)
//   rec_done    what cindm_ddpm1d_recorder_info reports
static int64_t rec_records(int64_t n, int every) { return (n + every - 1) / every; }

static int rec_begin(ChainArmed& took, const float* x, int n_steps, int64_t fpr, const char* x0_refusal = nullptr) {
    if (!took.rec.on()) return 0;
    RecSpec& r = took.rec;
    REQUIRE(n_steps >= 1 && fpr > 0, "recorder: empty chain");
    REQUIRE(((uintptr_t)x & 15) == 0, "recorder: the state x must be 16-byte aligned (the record node reads it 16 bytes per lane)");
    r.every = std::min(r.every, n_steps);      // the same records (every >= n: the result alone), and the kernel's step arithmetic stays small
    if ((r.streams & 2) && x0_refusal) return fail(x0_refusal);
    REQUIRE((fpr & 3) == 0, "recorder: the state's float count must be a multiple of 4");
    const int ns = (r.streams & 1) + ((r.streams >> 1) & 1);
    const int64_t need = (rec_records(n_steps, r.every) * ns + ((r.streams & 2) ? 1 : 0)) * fpr;
    if (r.buf_floats < need)
        return fail("recorder: buffer too small: " + std::to_string(r.buf_floats) + " floats, this chain needs " + std::to_string(need) +
                    " (ceil(steps / every) records x streams x floats per record, plus one staging record for x0)");
    r.n = n_steps; r.fpr = fpr;
    r.x0_stage = (r.streams & 2) ? r.buf + rec_records(n_steps, r.every) * ns * fpr : nullptr;
    took.h->rec = &took.rec;
    return 0;
}

// chain_record_kernel's store flavour: nt (1), the lowest of the three in both measured sessions, all three inside the spread of a 2-D
// step (DESIGN 4.5l).  Only the profiling build reads CINDM_RECORD_STORE = 0 (plain) / 1 / 2 (sc1), so that tools/bench_record.py
// can take that measurement again; the production library has no such switch.
static int rec_store_policy() {
#ifdef CINDM_PHASE_PROF
    const char* e = getenv("CINDM_RECORD_STORE");
    const int v = e ? atoi(e) : 1;
    if (v >= 0 && v <= 2) return v;
#endif
    return 1;
}

// t0 >= 0: a DDPM loop from that timestep (word = the timestep's word); -1: a DDIM loop (word = the step index's word)
static void rec_arm(cindm_ddpm1d* h, int t0, int word, int slot_stride, hipStream_t stream) {
    if (!h->rec) return;
    const RecSpec& r = *h->rec;
    RecordDesc d;
    d.dst = r.buf; d.fpr = r.fpr; d.every = r.every; d.n = r.n; d.streams = r.streams; d.t0 = t0;
    d.word = word; d.slot_stride = slot_stride; d.store = rec_store_policy(); d.pad = 0;
    hipLaunchKernelGGL(record_arm_kernel, dim3(1), dim3(64), 0, stream, h->t_dev, d);
}

static int rec_node(cindm_ddpm1d* h, const float* state, int slot, hipStream_t stream) {
    const RecSpec& r = *h->rec;
    const int ns = (r.streams & 1) + ((r.streams >> 1) & 1);
    const int64_t blocks = (r.fpr / 4 + kRecordThreads - 1) / kRecordThreads;
    hipLaunchKernelGGL(chain_record_kernel, dim3((unsigned)std::min<int64_t>(blocks, 2048), ns), dim3(kRecordThreads), 0, stream,
                       (const int*)h->t_dev, state, slot);
    HIPCHK(hipGetLastError());
    return 0;
}

static int rec_done(ChainArmed& took, int rc) {
    if (took.rec.on() && rc == 0) {
        const RecSpec& r = took.rec; int* info = took.h->rec_info;
        info[0] = (int)rec_records(r.n, r.every); info[1] = (int)r.fpr; info[2] = r.n; info[3] = r.streams;
    }
    return rc;
}

extern "C" int cindm_ddpm1d_set_recorder(cindm_ddpm1d* h, float* buf, int64_t buf_floats, int32_t every, int32_t streams) {
    if (h) h->armed.rec = RecSpec();      // (a refused call leaves the handle disarmed)
    if (buf) {
        REQUIRE(every >= 1, "recorder: every must be >= 1");
        REQUIRE(streams >= 1 && (streams & ~3) == 0, "recorder: unknown stream bit (1 = x, 2 = x0)");
        REQUIRE(buf_floats > 0 && ((uintptr_t)buf & 15) == 0, "recorder: the buffer must be 16-byte aligned and not empty");
    }
    REQUIRE(h, "null handle");
    if (!buf) return 0;
    RecSpec& r = h->armed.rec;
    r.buf = buf; r.buf_floats = buf_floats; r.every = every; r.streams = streams;
    return 0;
}

extern "C" int cindm_ddpm1d_recorder_info(const cindm_ddpm1d* h, int32_t info[4]) {
    REQUIRE(h && info, "null argument");
    for (int i = 0; i < 4; ++i) info[i] = h->rec_info[i];
    return 0;
}

// ---- the table objectives: waypoint (DESIGN 4.5m), quadratic (4.5q), pair-distance (4.5s) ----------------------------------------------
// cindm_ddpm1d_set_design_tables / _quadratic / _pairdist arm the handle, one slot per kind.  An entry either refuses the tables it
// took (design_refuse, through refuse_all_but: every chain that is not guided) or checks them against its descriptor and state
// (design_begin) and runs with the kind its descriptor's mode reads -- mode 7, the sum, with every kind armed: run_step reads h->dzt
// for the whole call, the re-run included.
// What differs between the kinds is data: the modes that read them, how messages name the kind and its two tables, what `width`
// counts, the alignment the update kernel needs and the ComposeArgs operands the tables become.
struct DesignKind {
    int mode_lo, mode_hi; const char* modes;               // the descriptor modes that read these tables, and as messages write them
    const char* label;                                     // the kind in messages
    const char* a_name; const char* b_name;                // its two tables
    const char* reads;                                     // the two as "mode N reads .. from tables" names them
    const char* setter;
    const char* noun; int per_body; const char* fits;      // width: what it counts, how many a body has, what it is held against
    const char* rows_rule; const char* width_rule;         // the setter's range refusals (the setter states the width's range itself)
    int align;                                             // bytes, of both tables
    const char* readers;                                   // who reads them, as the refusal of every other entry says it
    const char* lower_modes;                               // armed under a mode below its own: what those modes are
    const char* armed_as; const char* tables_of;           // armed under a mode above its own: its name there / as such a refusal names that mode's reader
    const float* ComposeArgs::*arg_a; const float* ComposeArgs::*arg_b;
};
static const DesignKind kDesignKinds[kNumDesignKinds] = {
    {3, 4, "3 / 4", "design tables", "target", "scale", "its target and scale", "cindm_ddpm1d_set_design_tables",
     "bodies", 1, "the composition has ", "rows, n_bodies and batch must be >= 1", "rows, n_bodies and batch must be >= 1", 16,
     "guided chains", "1 / 2 (the point objective, which reads none)", "design tables (target, scale)", nullptr,
     &ComposeArgs::dz_target, &ComposeArgs::dz_scale},
    {5, 5, "5", "quadratic design tables", "S", "h", "S and h", "cindm_ddpm1d_set_design_quadratic",
     "features", 4, "the composition's state has ", "rows and batch must be >= 1", "features must be a multiple of 4 in 4 .. 32", 16,
     "guided 1-D chains", "1 .. 4 (the point and waypoint objectives, which do not read them)", "quadratic design tables",
     "quadratic tables of cindm_ddpm1d_set_design_quadratic", &ComposeArgs::dz_S, &ComposeArgs::dz_h},
    {6, 6, "6", "pair-distance design tables", "band", "weight", "band and weight", "cindm_ddpm1d_set_design_pairdist",
     "bodies", 1, "the composition has ", "rows and batch must be >= 1", "n_bodies must be in 2 .. 8", 4,
     "guided 1-D chains", "1 .. 5 (the point, waypoint and quadratic objectives, which do not read them)", nullptr,
     "pair-distance tables of cindm_ddpm1d_set_design_pairdist", &ComposeArgs::dz_band, &ComposeArgs::dz_weight},
};

// the descriptor mode that reads every armed kind: the sum of the table objectives (DESIGN 4.5t)
constexpr int kDesignSumMode = 7;

// the kind whose tables a descriptor mode reads, or -1 (the point objective's modes read none; the sum's mode reads every armed kind)
static int design_kind_of(int mode) {
    for (int kind = 0; kind < kNumDesignKinds; ++kind)
        if (mode >= kDesignKinds[kind].mode_lo && mode <= kDesignKinds[kind].mode_hi) return kind;
    return -1;
}

static int design_refuse(const ChainArmed& took) {
    for (int kind = 0; kind < kNumDesignKinds; ++kind) {
        const DesignKind& k = kDesignKinds[kind];
        if (took.tables[kind].on())
            return fail(std::string(k.label) + ": only the " + k.readers + " (cindm_ddpm1d_sample_guided / _sample_ddim_guided) read them; the tables were dropped");
    }
    return 0;
}

// For each kind: when it serves dz->mode it must be armed and fit the state, otherwise it must not be armed.  Mode 7 (the sum, DESIGN
// 4.5t) is served by every kind: each armed one must fit the state, by that kind's own messages, and at least one must be armed; its
// last_n_step names the waypoint term's norm (1 = L2, 2 = L2square) and is read only when waypoint tables are armed.
// x, x2: the state buffers the guided update reads a row of as float4 (x2: the guided DDIM chain's second buffer, or null)
static int design_begin(ChainArmed& took, const cindm_design_desc* dz, int Ltot, int n_bodies, int64_t B, const float* x, const float* x2) {
    for (int kind = 0; kind < kNumDesignKinds; ++kind) {
        const DesignKind& k = kDesignKinds[kind]; DesignTables& t = took.tables[kind];
        const std::string label = k.label;
        if (dz->mode == kDesignSumMode) {
            if (!t.on()) continue;
            if (kind == kWaypoint && dz->last_n_step != 1 && dz->last_n_step != 2)
                return fail("design objective mode 7 with design tables armed: last_n_step names the waypoint term's norm, 1 (L2) or 2 (L2square), not " +
                            std::to_string(dz->last_n_step) + "; the tables were dropped");
        } else if (design_kind_of(dz->mode) != kind) {
            if (!t.on()) continue;
            if (dz->mode > k.mode_hi)
                return fail(std::string(k.armed_as) + " are armed but the descriptor's mode is " + std::to_string(dz->mode) + ", which reads the " +
                            kDesignKinds[design_kind_of(dz->mode)].tables_of + "; the tables were dropped");
            return fail(label + " are armed but the descriptor's mode is " + k.lower_modes + "; the tables were dropped");
        } else if (!t.on()) {
            return fail(std::string("design objective mode ") + k.modes + " reads " + k.reads + " from tables: arm them with " + k.setter + " before the chain call");
        }
        if (t.rows != Ltot)
            return fail(label + ": " + std::to_string(t.rows) + " rows, the state has " + std::to_string(Ltot));
        if (t.width != k.per_body * n_bodies)
            return fail(label + ": " + std::to_string(t.width) + " " + k.noun + ", " + k.fits + std::to_string(k.per_body * n_bodies));
        if (t.batch != B)
            return fail(label + ": made for a batch of " + std::to_string(t.batch) + ", the chain runs " + std::to_string(B));
        if ((((uintptr_t)t.a | (uintptr_t)t.b) & (uintptr_t)(k.align - 1)) != 0)
            return fail(label + ": " + k.a_name + " and " + k.b_name + " must be " + std::to_string(k.align) + "-byte aligned");
        if (kind == kQuadratic)
            REQUIRE((((uintptr_t)x | (uintptr_t)x2) & 15) == 0, "quadratic design tables: the state x must be 16-byte aligned (the update reads its rows 16 bytes at a time)");
        t.taken = true;
        took.h->dzt = took.tables;
    }
    if (dz->mode == kDesignSumMode) {
        bool any = false;
        for (const DesignTables& t : took.tables) any = any || t.taken;
        REQUIRE(any, "design objective mode 7 sums the table objectives armed on the handle: arm at least one with cindm_ddpm1d_set_design_tables, "
                     "_set_design_quadratic or _set_design_pairdist before the chain call");
    }
    return 0;
}

static void design_key(KeyBuilder& K, const cindm_ddpm1d* h) {
    for (int kind = 0; h->dzt && kind < kNumDesignKinds; ++kind) {
        const DesignTables& t = h->dzt[kind];
        if (t.taken) K(kind)(t.a)(t.b)(t.a_per_design)(t.b_per_design);
    }
}

// what the three setters share; width_ok: the setter's own rule for the width
static int design_arm(cindm_ddpm1d* h, int kind, const float* a, int32_t a_per_design, const float* b, int32_t b_per_design, int32_t rows,
                      int32_t width, bool width_ok, int64_t batch) {
    const DesignKind& k = kDesignKinds[kind];
    if (h) h->armed.tables[kind] = DesignTables();      // (a refused call leaves the handle disarmed)
    REQUIRE(h, "null handle");
    if (!a && !b) return 0;
    if (!a || !b) return fail(std::string(k.label) + ": " + k.a_name + " and " + k.b_name + " come together (NULL, NULL disarms)");
    if (rows < 1 || batch < 1) return fail(std::string(k.label) + ": " + k.rows_rule);
    if (!width_ok) return fail(std::string(k.label) + ": " + k.width_rule);
    DesignTables& t = h->armed.tables[kind];
    t.kind = kind; t.a = a; t.b = b; t.a_per_design = a_per_design ? 1 : 0; t.b_per_design = b_per_design ? 1 : 0;
    t.rows = rows; t.width = width; t.batch = batch;
    return 0;
}

extern "C" int cindm_ddpm1d_set_design_tables(cindm_ddpm1d* h, const float* target, int32_t target_per_design, const float* scale,
                                              int32_t scale_per_design, int32_t rows, int32_t n_bodies, int64_t batch) {
    return design_arm(h, kWaypoint, target, target_per_design, scale, scale_per_design, rows, n_bodies, n_bodies >= 1, batch);
}

extern "C" int cindm_ddpm1d_set_design_quadratic(cindm_ddpm1d* h, const float* S, int32_t S_per_design, const float* hvec,
                                                 int32_t h_per_design, int32_t rows, int32_t features, int64_t batch) {
    return design_arm(h, kQuadratic, S, S_per_design, hvec, h_per_design, rows, features, features >= 4 && features <= 32 && (features & 3) == 0, batch);
}

extern "C" int cindm_ddpm1d_set_design_pairdist(cindm_ddpm1d* h, const float* band, int32_t band_per_design, const float* weight,
                                                int32_t weight_per_design, int32_t rows, int32_t n_bodies, int64_t batch) {
    return design_arm(h, kPairDist, band, band_per_design, weight, weight_per_design, rows, n_bodies, n_bodies >= 2 && n_bodies <= 8, batch);
}

// ---- the known region of the 2-D chains (DESIGN 4.5n) ----------------------------------------------------------------------------------
// cindm_ddpm1d_set_known2d arms the handle; an entry either refuses the region it took (refuse_all_but: every 1-D chain) or checks it
// against its state (known2_begin, ddpm2d_host.inc) and runs with it: the chain body and the captured step read h->kn for the whole
// call, the re-run included.
extern "C" int cindm_ddpm1d_set_known2d(cindm_ddpm1d* h, const float* known, const uint8_t* mask, const float* noise_init_state,
                                        const float* noise_init_boundary, const float* noise_state_steps,
                                        const float* noise_boundary_steps, int64_t state_step_stride, int64_t boundary_step_stride,
                                        int64_t images, int32_t hw, int32_t cp) {
    if (h) h->armed.kn = Known2D();      // (a refused call leaves the handle disarmed)
    REQUIRE(h, "null handle");
    if (!known && !mask) return 0;
    REQUIRE(known && mask, "known region: values and mask come together (NULL, NULL disarms)");
    REQUIRE(images >= 1 && hw >= 1 && cp >= 4 && (cp & 3) == 0, "known region: images and hw must be >= 1, cp a multiple of 4");
    const int tapes = (noise_init_state != nullptr) + (noise_init_boundary != nullptr) + (noise_state_steps != nullptr) + (noise_boundary_steps != nullptr);
    REQUIRE(tapes == 0 || tapes == 4, "known region: the four noise tapes come together (all NULL: the counter-based generator)");
    REQUIRE(tapes == 0 || (state_step_stride >= 0 && boundary_step_stride >= 0), "known region: negative tape stride");
    for (const void* p : {(const void*)known, (const void*)mask, (const void*)noise_init_state, (const void*)noise_init_boundary,
                          (const void*)noise_state_steps, (const void*)noise_boundary_steps})
        REQUIRE(((uintptr_t)p & 15) == 0, "known region: values, mask and tapes must be 16-byte aligned");
    Known2D& k = h->armed.kn;
    k.known = known; k.mask = mask; k.zi_state = noise_init_state; k.zi_bound = noise_init_boundary;
    k.z_state = noise_state_steps; k.z_bound = noise_boundary_steps; k.zs_stride = state_step_stride; k.zb_stride = boundary_step_stride;
    k.images = images; k.hw = hw; k.cp = cp;
    return 0;
}

// ---- the known region of the 1-D chains (DESIGN 4.5o) ----------------------------------------------------------------------------------
// cindm_ddpm1d_set_known1d arms the handle; an entry either refuses the region it took (refuse_all_but with the entry's reason: the
// rollout, the time composition, the Langevin chain, every 2-D chain) or checks it against its state (known1_begin, ddpm1d_host.inc)
// and runs with it: the chain body and run_step read h->kn1 for the whole call, the re-run included.
extern "C" int cindm_ddpm1d_set_known1d(cindm_ddpm1d* h, const float* known, int32_t known_per_design, const uint8_t* mask,
                                        int32_t mask_per_design, const float* noise_init, const float* noise_steps,
                                        int64_t step_stride, const float* noise_recur, int64_t recur_stride, int32_t apply_init,
                                        int64_t batch, int32_t rows, int32_t feats) {
    if (h) h->armed.kn1 = Known1D();      // (a refused call leaves the handle disarmed)
    REQUIRE(h, "null handle");
    if (!known && !mask) return 0;
    REQUIRE(known && mask, "known region (1-D): values and mask come together (NULL, NULL disarms)");
    REQUIRE(batch >= 1 && rows >= 1 && feats >= 4 && (feats & 3) == 0, "known region (1-D): batch and rows must be >= 1, the features a multiple of 4");
    REQUIRE(!noise_recur || noise_steps, "known region (1-D): a relaxation tape comes with a step tape");
    REQUIRE(!noise_steps || noise_init || !apply_init, "known region (1-D): a step tape comes with the init tape (all NULL: the counter-based generator)");
    REQUIRE(!noise_init || noise_steps, "known region (1-D): the init tape comes with a step tape");
    REQUIRE(step_stride >= 0 && recur_stride >= 0, "known region (1-D): negative tape stride");
    for (const void* p : {(const void*)known, (const void*)mask, (const void*)noise_init, (const void*)noise_steps, (const void*)noise_recur})
        REQUIRE(((uintptr_t)p & 15) == 0, "known region (1-D): values, mask and tapes must be 16-byte aligned");
    Known1D& k = h->armed.kn1;
    k.known = known; k.mask = mask; k.known_per_design = known_per_design ? 1 : 0; k.mask_per_design = mask_per_design ? 1 : 0;
    k.z_init = noise_init; k.z_step = noise_steps; k.z_recur = noise_recur; k.step_stride = step_stride; k.recur_stride = recur_stride;
    k.batch = batch; k.rows = rows; k.feats = feats; k.apply_init = apply_init ? 1 : 0;
    return 0;
}

// ---- the second-order multistep solver (DESIGN 4.5r) -----------------------------------------------------------------------------------
// cindm_ddpm1d_set_multistep arms the handle; an entry either refuses the solver it took (refuse_all_but: every chain that is not one
// of the four DDIM chains) or checks it against its schedule and state (ms_begin) and runs with it: the DDIM update of step i adds
// kappa[i] (X_i - X_{i-1}) to its value and writes X_i to the history.  kappa[i] == 0 does not read the history: the first step of
// a chain, and of its recovery re-run, needs none.
// n_steps, coefs: the DDIM call's; state_floats, x, x2: the chain's state (x2: a second state buffer the update may read, or null)
static int ms_begin(ChainArmed& took, int32_t n_steps, const float* coefs, int64_t state_floats, const float* x, const float* x2 = nullptr) {
    if (!took.ms.on()) return 0;
    const Multistep& m = took.ms;
    if ((int64_t)m.kappa.size() != (int64_t)n_steps)
        return fail("multistep solver: armed for " + std::to_string(m.kappa.size()) + " steps, the chain runs " + std::to_string(n_steps));
    if (m.hist_floats != state_floats)
        return fail("multistep solver: the history holds " + std::to_string(m.hist_floats) + " floats, the chain's state " + std::to_string(state_floats));
    for (int i = 0; i < n_steps; ++i)
        REQUIRE(coefs[3 * i + 2] == 0.f, "multistep solver: every step's sigma must be zero (ddim_sampling_eta = 0: the solver is deterministic)");
    REQUIRE(m.hist != x && m.hist != x2, "multistep solver: the history may not be a state buffer of the chain");
    took.h->ms = &took.ms;
    return 0;
}

// (nothing armed: the key is what it was)
static void ms_key(KeyBuilder& K, const cindm_ddpm1d* h) {
    if (h->ms) K(1)(h->ms->hist);
}

extern "C" int cindm_ddpm1d_set_multistep(cindm_ddpm1d* h, const float* kappa_host, int32_t n_steps, float* hist, int64_t hist_floats) {
    if (h) h->armed.ms = Multistep();      // (a refused call leaves the handle disarmed)
    REQUIRE(h, "null handle");
    if (!kappa_host) return 0;
    REQUIRE(n_steps >= 1, "multistep solver: n_steps must be >= 1");
    REQUIRE(hist && hist_floats > 0 && ((uintptr_t)hist & 15) == 0, "multistep solver: the history must be 16-byte aligned and not empty");
    for (int i = 0; i < n_steps; ++i) REQUIRE(std::isfinite(kappa_host[i]), "multistep solver: kappa must be finite");
    Multistep& m = h->armed.ms;
    m.kappa.assign(kappa_host, kappa_host + n_steps); m.hist = hist; m.hist_floats = hist_floats;
    return 0;
}

// ---- what an entry does not serve -------------------------------------------------------------------------------------------------------
int ChainArmed::refuse_all_but(unsigned serves, const char* why_known1) const {
    if (!(serves & kServesTables) && design_refuse(*this) != 0) return -1;
    if (!(serves & kServesKnown2))
        REQUIRE(!kn.on(), "known region: only the 2-D chains (cindm_ddpm2d_sample / _sample_ddim / _sample_force / _sample_ddim_force) hold one; "
                          "the 1-D chains inpaint through their own arguments (inpaint_cond, initial_state_overwrite); the region was dropped");
    if (!(serves & kServesKnown1) && kn1.on())
        return fail(std::string("known region (1-D): ") + (why_known1 ? why_known1 : "this chain holds none") + "; the region was dropped");
    if (!(serves & kServesMultistep))
        REQUIRE(!ms.on(), "multistep solver: only the DDIM chains (cindm_ddpm1d_sample_ddim / _sample_ddim_guided, cindm_ddpm2d_sample_ddim / "
                          "_sample_ddim_force) run it; the solver was dropped");
    return 0;
}
