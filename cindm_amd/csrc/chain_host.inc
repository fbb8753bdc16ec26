// The chain driver: what every sampling entry (cindm_ddpm1d_sample*, cindm_ddpm2d_sample*) does around its own step.
// Textually included by cindm_hip.hip after struct cindm_ddpm1d and before the 2-D host files; each piece exists once.
//   chain_stream        which stream a chain runs on
//   stream_steps        the eager loop
//   graph_capture/_run  capture a step functor into an instantiated graph; launch it n times and synchronise
//   replay_once         the 2-D chains' replay: stream_steps, or capture + run + destroy (no cache)
//   upload_ddim_tables  schedule check + the DDIM loops' per-step device tables
// The 1-D replay (replay_steps in cindm_hip.hip: graph cached in the handle by key, ping-pong pair + odd tail, flag polls) is built
// on the same two graph functions.

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
