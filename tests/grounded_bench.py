"""Cost of grounded decoding on Groma-7B (random init): generate() ms/token at 4 rows and the batcher's tick at 64 rows, with no row
and with every row grounded, and the grammar kernel beside the sampler kernel at 64 rows.
   python tests/grounded_bench.py [--repeats 3]
Runs on a tree without the feature too (it then prints the plain numbers only), so two checkouts can be alternated."""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from groma_amd import config, constants, ops, synth
from groma_amd.groma import GromaModel
from groma_amd.serving import ContinuousBatcher

HAVE = hasattr(ops, "grammar_step")
REPEATS = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 3
cfg = config.groma_7b(box_score_thres=0.0)
m = GromaModel.from_synthetic(cfg, seed=0, device='cuda')
m.init_special_token_id(constants.SyntheticTokenizer())
m.generation_config.eos_token_id = None   # random weights: never stop early
tag = "grounded tree" if HAVE else "plain tree"


def gen_ms_per_token(**kw):
    images, ids = synth.make_inputs(cfg, m, 4, seed=5)
    images, ids = images.cuda(), ids.cuda()
    dt = {}
    for new in (1, 33, 1, 33):   # (the first pair warms up and captures)
        torch.manual_seed(0); torch.cuda.synchronize(); t = time.perf_counter()
        m.generate(ids, images=images, max_new_tokens=new, **kw); torch.cuda.synchronize()
        dt[new] = time.perf_counter() - t
    return (dt[33] - dt[1]) / 32 * 1e3


def replay_ms(g, n=50):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n):
        g.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


for rep in range(REPEATS):
    line = f"[{tag}] generate, 4 rows, graph step: none grounded {gen_ms_per_token():.3f} ms/token"
    if HAVE:
        line += f"; all grounded {gen_ms_per_token(grounded=True):.3f} ms/token"
    print(line, flush=True)

b = ContinuousBatcher(m, max_rows=64, max_len=1024, **({"grounded": True} if HAVE else {}))
b.step()   # capture
for rep in range(REPEATS):
    line = f"[{tag}] batcher tick, 64 rows: plain graph {replay_ms(b.graph):.4f} ms"
    if HAVE:
        for name, s in (("TEXT", 0), ("BODY", 2)):
            b.gstate.fill_(s); b.gn.fill_(40); b.tok.fill_(17)
            line += f"; grounded graph, every row {name} {replay_ms(b.graph_g):.4f} ms"
        b.gstate.fill_(-1)
        line += f"; grounded graph, no row grounded {replay_ms(b.graph_g):.4f} ms"
    print(line, flush=True)

if HAVE:   # the kernels alone: 50 launches per captured graph, on the tick's own logits buffer
    logits = m.llm.decode_logits(64)
    nxt = torch.zeros((64,), dtype=torch.int64, device='cuda')

    def per_launch_us(fn):
        fn(); torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(50):
                fn()
        return min(replay_ms(g, 20) for _ in range(3)) / 50 * 1e3
    for rep in range(REPEATS):
        line = f"[{tag}] kernels, 64 rows, V={m.llm.V}: "
        logits.normal_()
        line += f"sample_rows {per_launch_us(lambda: ops.sample_rows(logits, m.llm.V, b.inv_temp, b.seed, pos=b.pos, pos_stride=1, pos_off=1, out=nxt)):.2f} us"
        for name, s in (("TEXT", 0), ("OPEN", 1), ("BODY", 2), ("unconstrained", -1)):
            b.gstate.fill_(s); b.gn.fill_(40); b.tok.fill_(17)
            line += f"; grammar_step {name} {per_launch_us(lambda: ops.grammar_step(logits, m.llm.V, b.gstate, b.gn, b.gids, last_tok=b.tok)):.2f} us"
        print(line, flush=True)
