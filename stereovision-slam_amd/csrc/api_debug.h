// api_debug.h — included by svslam_hip.hip.  Entry points: svslam_set_host_threads, svslam_debug_host_ns, svslam_debug_hold_cus,
// svslam_debug_clock_mhz with their two kernels.  Owns of svslam_ctx: pool; reads host_ns.

extern "C" {

// number of host threads the library may use to prepare batched calls (BA structure
// building is per problem and independent); default 1
int svslam_set_host_threads(svslam_ctx *c, int n)
{
    c->pool.reset(n > 1 ? new svs::ThreadPool(n) : nullptr);
    return 0;
}

// test hook: host-side wall time per category since the last call (ns):
// 0 h2d enqueue, 1 d2h enqueue, 2 stream wait, 5 event collection; slot 6 is a count: local-BA problems solved by the
// low-latency path (one problem over several workgroups)
int svslam_debug_host_ns(svslam_ctx *c, long long *out8)
{
    c->host_ns[7] = c->ll.fallbacks; c->ll.fallbacks = 0;      // slot 7: problems the low-latency solver gave up on, repeated by the batch solver
    for (int i = 0; i < 8; ++i) { out8[i] = c->host_ns[i]; c->host_ns[i] = 0; }
    return 0;
}

// test hook: effective shader clock.  A single wave spins for ~`ms` milliseconds of
// wall_clock64 (100 MHz, constant) and reports the clock64() (shader cycles) it saw.
__global__ void k_clock_probe(long long *out, long long wall_ticks)
{
    long long w0 = wall_clock64(), c0 = clock64();
    long long w = w0;
    while (w - w0 < wall_ticks) w = wall_clock64();
    long long c1 = clock64();
    if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = w - w0; out[1] = c1 - c0; }
}
// test hook: `ncus` workgroups that each take a CU's whole LDS and spin for `ms` — the CUs they sit on cannot take a workgroup
// that needs LDS until they leave (what another process' kernels do to a partitioned or shared GPU).  Asynchronous: enqueued on
// the context's stream, returns at once; svslam_sync waits for it.
__global__ void k_hold_cu(long long wall_ticks)
{
    extern __shared__ unsigned char hold_lds[];
    if (threadIdx.x == 0) hold_lds[0] = 1;
    const long long w0 = wall_clock64();
    while (wall_clock64() - w0 < wall_ticks) __builtin_amdgcn_s_sleep(8);
}
int svslam_debug_hold_cus(svslam_ctx *c, int ncus, double ms)
{
    if (ncus <= 0) return 0;
    const int lds = 160 * 1024;
    HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_hold_cu), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(k_hold_cu, dim3(ncus), dim3(64), lds, c->stream, (long long)(ms * 1e5));
    HIPCHK(c, hipGetLastError());
    return 0;
}

int svslam_debug_clock_mhz(svslam_ctx *c, int blocks, double ms, double *mhz)
{
    long long *d = nullptr, h[2] = { 0, 0 };
    HIPCHK(c, hipMalloc(&d, 16));
    hipLaunchKernelGGL(k_clock_probe, dim3(blocks), dim3(64), 0, c->stream, d, (long long)(ms * 1e5));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, d, 16, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    *mhz = h[0] > 0 ? 100.0 * (double)h[1] / (double)h[0] : 0.0;
    return 0;
}

} // extern "C"
