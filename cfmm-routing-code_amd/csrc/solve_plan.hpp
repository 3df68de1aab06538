// Which of the first-order solve's host drivers runs a solve, and under which envelope: a pure function of a handful of facts about
// the context, the options and three process-wide A/B switches.  Host only: nothing of HIP, nothing of cfmm_ctx -- cfmm_hip.hip
// (solve_lbfgs) gathers the facts, tests/test_host.py walks the whole table.
#pragma once

struct PlanFacts {
    bool tiny_applies;       // one workgroup holds the whole solve (tiny.hpp)
    bool fused_applies;      // the update fits the evaluation launch (iterate.hpp)
    bool sharded;            // pool-sharded: a communicator and / or an attached one-shot exchange
    int n_ranks;
    bool oneshot_runahead;   // the one-shot exchange's collectives can be skipped on the device: the host may run ahead
    bool multi_graph;        // CFMM_MULTI_GRAPH: capture the pool-sharded iterations too
    bool os_ready;           // a one-shot exchange is attached
    bool no_graph;           // CFMM_NO_GRAPH
    bool det;                // the reproducible mode
    int iters_per_graph;     // as the caller set it
    int max_evals;
    // read once per process (A/B switches)
    bool fused_graph;        // CFMM_FUSED_GRAPH != 0: replay the one-launch iterations from a graph
    bool zero_copy_off;      // CFMM_ZERO_COPY == 0: copy the result back instead of letting the kernels store it in pinned memory
    bool envelope_classic;   // CFMM_ENVELOPE=classic: the synchronised envelope
};

enum class Drive {
    Tiny,          // one launch of solve_tiny_kernel
    Eager,         // one iter_kernel launch per iteration, the host a few launches ahead of a pinned progress word
    RingChunks,    // RCCL: chunks of iter_kernel launches, the decision one chunk behind on the pinned progress ring
    Chunks         // graph replay or eager enqueue in chunks, a state copy and an event per chunk
};

struct FirstOrderPlan {
    Drive drive;
    bool fused;              // iter_kernel, not the two-launch iteration
    bool use_graph;          // the chunks are replayed from the captured graph
    bool zero_copy;          // the kernels leave the result in pinned memory themselves
    bool sealed;             // ... and the host neither synchronises the stream nor records events around the solve (iterate.hpp: EnvRec)
    int iters_per_graph;     // adjusted: what the graph cache is keyed on
};

inline FirstOrderPlan plan_first_order(const PlanFacts &f)
{
    FirstOrderPlan p;
    const bool tiny = f.tiny_applies;
    p.fused = !tiny && f.fused_applies;
    p.iters_per_graph = f.iters_per_graph;
    if (p.fused) p.iters_per_graph = (p.iters_per_graph + 2) / 3 * 3;      // the rotation phase t % 3 is baked into captured launches
    // pool-sharded through RCCL: the chunked scheme polls one chunk behind, so a solve leaves up to two chunks of iterations
    // -- each with a live collective and RCCL's ~35 us of host time per call -- behind its end: short chunks
    // (a one-rank communicator's collective is free: there the polls cost more than the idle iterations, 0.79 vs 0.75 ms)
    if (f.sharded && f.n_ranks > 1 && !f.oneshot_runahead && !f.multi_graph) p.iters_per_graph = 3;
    // Single GPU: `iters_per_graph` iterations are replayed from one captured hipGraph.  Pool-sharded (RCCL all-reduce inside every
    // iteration): the same iterations are enqueued eagerly, the way RCCL is conventionally driven (CFMM_MULTI_GRAPH=1 opts into
    // capturing them too).  The one-launch iteration is replayed from a graph only when asked to (A/B)
    const bool graph_opt = p.fused && !f.sharded && f.fused_graph;
    p.use_graph = !tiny && (!f.sharded || (f.multi_graph && !f.os_ready)) && !f.no_graph && (!p.fused || f.sharded || f.fused_graph);
    p.zero_copy = p.fused && !f.sharded && !graph_opt && !f.det && !f.zero_copy_off;
    p.sealed = p.zero_copy && !f.envelope_classic && f.max_evals < 0xffffff;      // (the words carry 24 bits of evaluation count)
    if (tiny) p.drive = Drive::Tiny;
    else if (p.fused && (!f.sharded || f.oneshot_runahead) && !graph_opt) p.drive = Drive::Eager;
    else if (p.fused && f.sharded && !p.use_graph) p.drive = Drive::RingChunks;
    else p.drive = Drive::Chunks;
    return p;
}
