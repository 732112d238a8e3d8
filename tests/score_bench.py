"""Cost of teacher-forced scoring: gr_label_logprob_rows beside the sampler's log-normaliser (gr_sample_rows_lp, k = 0, greedy) on
the same logits at 64 and at 14 x 582 rows of 32 128, and GromaModel.score() beside forward(labels=...) on the benchmark's 14-image
batch of Groma-7B (random init) with labels on the last 16 positions of every row: step time and peak allocated memory.
   python tests/score_bench.py [--repeats 3] [--kernels-only]"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groma_amd import config, constants, ops, synth
from groma_amd.constants import IGNORE_INDEX
from groma_amd.groma import GromaModel

REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
V, LD = 32128, 32128
STREAM_TBS = (6.0, 6.3)   # measured streaming-read rate of the chip (a float4 copy / an in-order sweep of a table beyond the caches)


def graph_us(fn, launches, replays=5):
    """device time of one launch: `launches` of them captured in one graph, the best of 3 timings of `replays` replays"""
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    best = float("inf")
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            g.replay()
        b.record(); torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / (replays * launches) * 1e3)
    return best


def kernels():
    for rows, launches in ((64, 50), (14 * 582, 4)):
        x = torch.empty((rows, LD), device="cuda").normal_() * 3.0
        labels = torch.randint(0, V, (rows,), device="cuda")
        inv, seed = torch.zeros((rows,), device="cuda"), torch.zeros((rows,), dtype=torch.int64, device="cuda")
        k, tok, lp = torch.zeros((rows,), dtype=torch.int32, device="cuda"), torch.empty((rows,), dtype=torch.int64, device="cuda"), torch.empty((rows,), device="cuda")
        lse, greedy, rank, out = (torch.empty((rows,), dtype=d, device="cuda") for d in (torch.float32, torch.int64, torch.int32, torch.float32))
        new = lambda: ops.label_logprob_rows(x, V, labels, lse=lse, greedy=greedy, rank=rank, out=out)
        old = lambda: ops.sample_rows_lp(x, V, inv, seed, out=tok, logprob=lp, k=k)
        new(); old(); torch.cuda.synchronize()
        # the same log-probability of the greedy token from both kernels (different summation orders: last bits only)
        diff = float((ops.label_logprob_rows(x, V, tok) - lp).abs().max())
        mb = rows * V * 4 / 1e6
        where = "cache-resident between launches (the rate is not an HBM rate)" if mb < 256 else "beyond the 256 MiB Infinity Cache: read from HBM"
        for rep in range(REPEATS):   # alternated
            t_new, t_old = graph_us(new, launches), graph_us(old, launches)
            rate = mb * 1e6 / (t_new * 1e-6) / 1e12   # TB/s
            print(f"[kernels] {rows} rows x {V} ({mb:.1f} MB, {where}): label_logprob_rows {t_new:.2f} us = {rate:.2f} TB/s read "
                  f"({rate / STREAM_TBS[1] * 100:.0f}-{rate / STREAM_TBS[0] * 100:.0f} % of the {STREAM_TBS[0]}-{STREAM_TBS[1]} TB/s streaming rate); "
                  f"sample_rows_lp k=0 {t_old:.2f} us = {mb * 1e6 / (t_old * 1e-6) / 1e12:.2f} TB/s; "
                  f"new / old {t_new / t_old:.3f}; max |logprob difference| {diff:.2e}", flush=True)
        del x


def model_step():
    cfg = config.groma_7b(box_score_thres=0.0)
    m = GromaModel.from_synthetic(cfg, seed=0, device="cuda")
    m.init_special_token_id(constants.SyntheticTokenizer())
    images, ids = synth.make_inputs(cfg, m, 14, seed=5)
    images, ids = images.cuda(), ids.cuda()
    labels = torch.full_like(ids, IGNORE_INDEX)
    labels[:, -16:] = ids[:, -16:]

    def run(fn, n):
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); ts = []
        for _ in range(n):
            torch.manual_seed(0); torch.cuda.synchronize(); t = time.perf_counter()
            r = fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return sorted(ts)[len(ts) // 2], torch.cuda.max_memory_allocated() / 2 ** 20, r

    score = lambda: m.score(ids, labels, images=images)
    fwd = lambda: m.forward(input_ids=ids, labels=labels, images=images)[0]
    run(score, 4), run(fwd, 4)   # warm-up: arenas grow, the prefill graphs are captured on the third sighting
    base = torch.cuda.memory_allocated() / 2 ** 20
    for rep in range(REPEATS):   # alternated
        ts, ms, o = run(score, 5)
        tf, mf, loss = run(fwd, 5)
        L = m._last_aux["input_ids"].shape[1]
        print(f"[step] 14 images, expanded length {L}, {int(o.num_tokens.sum())} scored labels: score() {ts:.1f} ms, peak {ms:.0f} MiB; "
              f"forward(labels=) {tf:.1f} ms, peak {mf:.0f} MiB (allocated at rest {base:.0f} MiB); peak difference {mf - ms:.0f} MiB, "
              f"full fp32 logits [14 x {L}, {m.llm.Vpad}] = {14 * L * m.llm.Vpad * 4 / 2 ** 20:.0f} MiB; "
              f"loss {float(o.loss):.6f} vs {float(loss):.6f}", flush=True)


if __name__ == "__main__":
    kernels()
    if "--kernels-only" not in sys.argv:
        model_step()
