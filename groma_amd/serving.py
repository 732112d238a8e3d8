"""Continuous-batch decode loop + KV-cache manager.

The reference serves one request at a time, one python-driven forward per token
(groma/serve/model_worker.py:287-338: prefill with `model(input_ids, images=..., use_cache=True)`, then
`model(input_ids=[[token]], past_key_values=...)` per token, arg-max / multinomial on the host, stop on EOS or a
stop id).  Decode is HBM-bound on the 13.2 GB weight stream, and that stream is shared by every row of
a step -- so the MI355X design batches the decode steps of *different requests*:

  * an arena of `max_rows` KV slots ([rows, H, max_len, hd] per layer, K and V^T) -- the KV manager hands a slot
    to a request at admission and takes it back when the request finishes; nothing is copied or compacted.  With
    `grow_to` the arena is re-allocated at a larger `max_len` (live rows copied, the step re-captured) when a request
    arrives that would not fit -- the reference's cache has no bound but the model's positions (model_worker.py:287-338);
  * the requests admitted in one tick are prefilled TOGETHER (one batched forward into a staging cache, then each row's KV is moved
    to its slot).  Every kernel of the path is row- / image-independent, so a row of that batch is bit-identical to a batch-1
    `GromaModel.forward` of the same request (tests/test_fullsize_properties_gpu.py) and independent of its company;
  * with `overlap_admission=True` (round 6) that prefill runs on a worker thread and a stream of its own while the decode ticks of
    the live rows go on: the prefill is compute-bound, the ticks stream weights, and the two share the chip (measured,
    profiles/r06_overlap_probe.txt: the same work finishes 1.12-1.16x sooner, and a live row waits <= 15 ms for its next token
    during an admission instead of the whole 50 ms prefill).  The rows join at the first tick after their prefill has finished;
    a request's tokens are the same either way (rows are independent);
  * every decode step advances ALL occupied rows with one captured hipGraph: per-row positions live on the device
    (`pos_dev`, stride 1 -- csrc/decode.hip), idle rows are masked, the host only reads back the `max_rows` new ids;
  * rows are computed independently by every kernel of the step (GEMV rows, per-(row, head) attention), so a
    request's tokens do not depend on its neighbours or on when it was admitted (tests/test_serving_gpu.py).

Ragged lengths are exact here: each row attends to its own [0, pos] -- the padded-prefix artefact of batched HF
generate cannot occur because rows are never padded against each other.

With `kv_pages=N` the arena is PAGED instead (engine.PagedKVCache): N pages of 64 positions per layer plus a sink page, and a
block table that maps each row's positions to pages.  A request reserves the pages of its context bound at admission, keeps those
its prompt and new tokens can reach, and gives them back when it finishes, so a fixed budget holds more and longer rows than
`max_rows` slots of `max_len` each.  Admission is FIFO and waits while the head request's pages are not free.

With `prefix_cache=True` on top (PrefixCache), a cold prompt's whole pages stay behind as an entry keyed by its image, boxes, seed and
precision.  A later request of the same key whose ids share the image prefix maps those pages below p0 (the last page boundary inside
the shared part) and prefills only [p0, L) on the pool (LlamaEngine.prefill_paged): the same tokens as a cold admission, without the
vision stages and the prefix prefill.  Nothing writes below p0, so shared pages never need a copy.
"""
import hashlib
import threading
from collections import OrderedDict, deque
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from . import engine, grammar, ops

I32, I64, F32 = torch.int32, torch.int64, torch.float32


class SlotTable:
    """KV-arena bookkeeping (host side, no device work): which row belongs to which request."""

    def __init__(self, n):
        self.n = n
        self.owner = [None] * n
        self._free = deque(range(n))

    def acquire(self, rid):
        if not self._free:
            return None
        s = self._free.popleft()
        self.owner[s] = rid
        return s

    def release(self, slot):
        if self.owner[slot] is None:
            raise ValueError(f"slot {slot} is not in use")
        self.owner[slot] = None
        self._free.append(slot)

    @property
    def n_free(self):
        return len(self._free)

    def active(self):
        return [s for s in range(self.n) if self.owner[s] is not None]


class PagePool:
    """Page bookkeeping of a paged KV cache (host side, no device work): pages 1..n are handed out, page 0 -- the sink page every
    unowned block-table entry points at -- never is.  A page may have several holders (live rows and prefix-cache entries that map
    it): retain() adds one, release() drops one and frees the page with its last."""

    def __init__(self, n):
        if n < 1:
            raise ValueError("a page pool needs at least one page")
        self.n = n
        self._free = deque(range(1, n + 1))
        self._used = set()
        self._ref = {}   # page -> holders (pages in use only)
        self.high_water = 0

    def reserve(self, k):
        """k page ids, or None (nothing taken) when fewer than k are free"""
        if k < 0:
            raise ValueError("negative page count")
        if k > len(self._free):
            return None
        ids = [self._free.popleft() for _ in range(k)]
        self._used.update(ids)
        self._ref.update((i, 1) for i in ids)
        self.high_water = max(self.high_water, len(self._used))
        return ids

    def retain(self, ids):
        """one more holder for each of `ids` (pages in use; an id listed twice gains two)"""
        ids = list(ids)
        if any(i not in self._used for i in ids):
            raise ValueError(f"pages {ids} are not all in use")
        for i in ids:
            self._ref[i] += 1

    def release(self, ids):
        """one holder fewer for each of `ids`; a page goes back to the free list with its last holder"""
        ids = list(ids)
        if len(set(ids)) != len(ids) or any(i not in self._used for i in ids):
            raise ValueError(f"pages {ids} are not all in use")
        for i in ids:
            self._ref[i] -= 1
            if self._ref[i] == 0:
                del self._ref[i]
                self._used.discard(i)
                self._free.append(i)

    def refs(self, i):
        """holders of page i (0: free)"""
        return self._ref.get(i, 0)

    @property
    def n_shared(self):
        """pages with more than one holder"""
        return sum(1 for v in self._ref.values() if v > 1)

    @property
    def n_free(self):
        return len(self._free)


def prefix_key(image, seed, refer_boxes=None, ground_boxes=None, precision=None):
    """what a prompt's image prefix depends on besides its ids: a digest of the image's bytes, the region-shuffle seed, the refer /
    ground boxes and the model's precision.  None (no cache entry can be shared) without an explicit seed."""
    if seed is None:
        return None
    h = hashlib.blake2b(digest_size=16)
    for t in (image, refer_boxes, ground_boxes):
        if t is None:
            h.update(b"none;")
            continue
        t = t.detach().to("cpu").contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return (h.hexdigest(), int(seed), str(precision))


@dataclass
class PrefixEntry:
    """one cached image prefix: the whole KV pages of a cold-admitted prompt and what a later suffix prefill needs again"""
    key: tuple
    ids: torch.Tensor            # un-expanded prompt ids (host)
    ids_x: torch.Tensor          # expanded ids (host)
    pred_boxes: torch.Tensor
    pages: List[int]             # the prompt's whole pages (positions [0, 64 * len(pages)))
    rows: Optional[torch.Tensor]  # f32 [L - e0, T]: the LLM input rows of positions [e0, L)
    e0: int                      # first position of the page that holds the last injected (image / region) row


@dataclass
class PrefixMatch:
    entry: PrefixEntry
    u: int     # common prefix of the un-expanded ids
    c: int     # its expanded length
    p0: int    # the suffix prefill starts here (a page boundary inside the shared prefix)
    L: int     # the request's expanded prompt length


class PrefixCache:
    """Host side of the prefix cache (no device work): entries in least-recently-used order, matching and eviction.  Entries hold
    their pages in the PagePool (retain / release), so a page an evicted entry shared stays allocated while a live row maps it."""

    def __init__(self, pool, placeholders, page=64):
        self.pool, self.placeholders, self.page = pool, frozenset(int(x) for x in placeholders), page
        self.entries = OrderedDict()   # id -> PrefixEntry, oldest use first
        self._next = 0
        self.evicted = 0

    def __len__(self):
        return len(self.entries)

    def match(self, key, ids):
        """the best entry of `key` for the un-expanded ids, or None (a miss).  The longest common prefix u of the ids must cover every
        placeholder of the request; it expands to c positions and the suffix prefill starts at p0 = the last page boundary <= c (and
        < L, the request's expanded length, so that at least its last position is computed); p0 = 0 is a miss."""
        if key is None:
            return None
        ids_l = ids.tolist()
        ph = [i for i, x in enumerate(ids_l) if x in self.placeholders]
        best = None
        for e in self.entries.values():
            if e.key != key:
                continue
            eu = e.ids.tolist()
            n = min(len(eu), len(ids_l))
            u = 0
            while u < n and eu[u] == ids_l[u]:
                u += 1
            if not ph or ph[-1] >= u:
                continue
            c = u + (len(e.ids_x) - len(eu))
            L = c + len(ids_l) - u
            p0 = self.page * (min(c, L - 1) // self.page)
            if p0 == 0 or p0 < e.e0 or p0 > self.page * len(e.pages):
                continue
            if best is None or (p0, u) > (best.p0, best.u):
                best = PrefixMatch(e, u, c, p0, L)
        return best

    def touch(self, e):
        for k, v in self.entries.items():
            if v is e:
                self.entries.move_to_end(k)
                return

    def add(self, key, ids, ids_x, pred_boxes, pages, rows, e0):
        """a new entry holding `pages` (retained here); an entry of the same key and ids is only touched"""
        for k, v in self.entries.items():
            if v.key == key and torch.equal(v.ids, ids):
                self.entries.move_to_end(k)
                return v
        self.pool.retain(pages)
        e = PrefixEntry(key, ids, ids_x, pred_boxes, list(pages), rows, int(e0))
        self.entries[self._next] = e
        self._next += 1
        return e

    def evict(self):
        """drop the least recently used entry (its pages lose one holder).  False when there is none."""
        if not self.entries:
            return False
        _, e = self.entries.popitem(last=False)
        self.pool.release(e.pages)
        self.evicted += 1
        return True

    def clear(self):
        while self.evict():
            pass


@dataclass
class Request:
    rid: int
    input_ids: torch.Tensor                 # [P] int64 (un-expanded prompt: <image> / <region> placeholders)
    image: torch.Tensor                     # [3, S, S] float
    max_new_tokens: int = 256
    refer_boxes: Optional[torch.Tensor] = None
    ground_boxes: Optional[torch.Tensor] = None
    eos_token_id: Optional[int] = None
    stop_token_id: Optional[int] = None     # model_worker.py:277-283 `stop` when it tokenises to one id
    seed: Optional[int] = None              # torch.manual_seed before the prefill (region shuffle); also keys the sampler
    temperature: float = 0.0                # model_worker.py:269,307-311: < 1e-4 -> arg-max, else softmax(logits / T) sampling
    tokens: List[int] = field(default_factory=list)
    pred_boxes: Optional[torch.Tensor] = None
    slot: Optional[int] = None
    prompt_len: int = 0                     # expanded length L in the cache
    done: bool = False
    error: Optional[str] = None
    pages: Optional[List[int]] = None       # paged mode: the pages reserved for this request (released when it finishes)
    hit: Optional["PrefixMatch"] = None     # prefix cache: the cached prefix this request's suffix prefill continues
    logprobs_k: Optional[int] = None        # submit(logprobs=): None = off, 0 = each token's log-probability, 1..8 = plus that many alternatives
    logprobs: Optional[List[float]] = None  # one per entry of `tokens` (natural log, softmax of the raw logits: temperature 1)
    top_logprobs: Optional[List[List[tuple]]] = None   # logprobs_k >= 1: per token, the k best (token id, log-probability), best first
    grounded: bool = False                  # submit(grounded=True): the region-token grammar (grammar.py) constrains every token
    grammar_state: Optional[int] = None     # grounded, once done: the state behind the last token (1 / 2: cut inside a region list)


class ContinuousBatcher:
    @engine.model_entry(lambda self, *a, **kw: (a[0] if a else kw["model"]).precision)
    def __init__(self, model, max_rows=8, max_len=1024, use_graph=True, grow_to=None, overlap_admission=None, admit_min=2, admit_hold=8,
                 kv_pages=None, admit_rows=None, max_prompt_len=None, prefix_cache=False, grounded=False):
        """kv_pages=N: a paged KV cache of N pages of 64 positions (engine.PagedKVCache) instead of max_rows slots of max_len positions;
        max_len is then the per-request cap.  admit_rows (default min(max_rows, 8)) bounds an admission wave, max_prompt_len (default
        min(max_len, 1024)) the prompt part of a request: the staging cache the prefills land in holds admit_rows x max_prompt_len.
        prefix_cache=True (paged mode only): requests with an explicit seed that share an image prefix with an earlier one map its
        whole KV pages and prefill only their suffix (see `_take_batch` / `_prefill_hits`).
        grounded=True: requests may ask for grounded decoding (submit(grounded=True), grammar.py).  The step is then also captured
        with gr_grammar_step between the head and the sampler, on per-row device state (`gstate`: -1 = not constrained, `gn`: the
        boxes of the row's image); those graphs are replayed on ticks where a live row is grounded, the plain ones otherwise."""
        if prefix_cache and kv_pages is None:
            raise ValueError("prefix_cache needs a paged KV cache (kv_pages=N): cached prefixes are shared as whole pages")
        if max_rows < 1 or max_rows > 64:
            raise ValueError("max_rows must be in 1..64 (1..8: the fused 8-row weight streams; 9..64: the matrix-unit weight streams, "
                             "csrc/gemm_skinny.hip / gemm_skinny_fp8.hip -- single-type 16-bit or e4m3 models; others fall back to the general kernels)")
        if max_len % 64 or max_len > 8192:
            raise ValueError("max_len must be a multiple of 64 and <= 8192")
        if grow_to is not None and (grow_to % 64 or grow_to < max_len or grow_to > 8192):
            raise ValueError("grow_to must be a multiple of 64 in max_len..8192")
        self.paged = kv_pages is not None
        if self.paged:
            self._check_paged(model, max_rows, max_len, grow_to, int(kv_pages))
        self.grow_to = int(grow_to or max_len)   # the arena may be re-allocated up to this many positions per slot (default: fixed)
        self.model, self.llm = model, model.llm
        self.rows, self.max_len, self.use_graph = max_rows, max_len, use_graph
        dev = model.device
        if self.paged:
            self.admit_rows = max(1, min(max_rows, int(admit_rows or min(max_rows, 8))))
            self.max_prompt_len = int(max_prompt_len or min(max_len, 1024))
            if self.max_prompt_len % 64 or not 0 < self.max_prompt_len <= max_len:
                raise ValueError("max_prompt_len must be a multiple of 64 in 64..max_len")
            self.pages = PagePool(int(kv_pages))
            with self.llm._st("attn"):
                self.arena = self.llm.new_paged_cache(max_rows, max_len, int(kv_pages), dev)
            self.staging = self.llm.new_cache(self.admit_rows, self.max_prompt_len, dev)
        else:
            self.admit_rows = max_rows
            self.arena = self.llm.new_cache(max_rows, max_len, dev)
            self.staging = self.llm.new_cache(max_rows, max_len, dev)  # batched prefills land here, then move to their slots
        self.slots = SlotTable(max_rows)
        # prefix cache: entries + LRU on the host; the admission table the suffix prefills address (never the live table the captured
        # step reads: a hit's row joins that one at placement)
        self.prefix, self.prefix_hits, self.prefix_misses = None, 0, 0
        if prefix_cache:
            ph = [model.img_token_id, model.reg_token_id, model.refer_box_token_id, model.ground_box_token_id,
                  model.refer_feat_token_id, model.pad_token_id]
            self.prefix = PrefixCache(self.pages, [x for x in ph if x is not None])
            self._inj = frozenset(int(x) for x in (model.img_token_id, model.reg_token_id, model.refer_feat_token_id) if x is not None)
            self._adm_table = torch.zeros((self.admit_rows, max_len // 64), dtype=I32, device=dev)
        self.queue = deque()
        self.live = {}
        self._next_rid = 0
        # device-resident loop state: one entry per row
        self.tok = torch.zeros((max_rows,), dtype=I64, device=dev)
        self.nxt = torch.zeros((max_rows,), dtype=I64, device=dev)
        self.occupied = torch.zeros((max_rows,), dtype=I64, device=dev)   # gr_greedy_advance `unfinished`
        self.pos = torch.zeros((max_rows,), dtype=I32, device=dev)  # idle rows rewrite position 0 of their own (free) slot
        self.step_ctr = torch.zeros((1,), dtype=I32, device=dev)
        self.n_live = torch.zeros((1,), dtype=I32, device=dev)
        self._seq = torch.zeros((max_rows, 1), dtype=I64, device=dev)
        self.h = torch.zeros((max_rows, self.llm.T), dtype=F32, device=dev)
        self.inv_temp = torch.zeros((max_rows,), dtype=F32, device=dev)   # per-row 1/temperature (0 = greedy)
        self.seed = torch.zeros((max_rows,), dtype=I64, device=dev)       # per-row sampler seed
        # per-token log-probabilities (gr_sample_rows_lp): lp_k[row] = -1 (the row does not ask: its sampler work is gr_sample_rows'),
        # 0 (the chosen token) or 1..8 (plus alternatives) -- device state, so rows that ask and rows that do not share one captured
        # step.  The three outputs are views of ONE buffer: a tick on which a live row asked fetches it with one copy.
        self.lp_k = torch.full((max_rows,), -1, dtype=I32, device=dev)
        self._lp_pack = torch.zeros((max_rows * 100,), dtype=torch.uint8, device=dev)
        self._lp_host = torch.zeros((max_rows * 100,), dtype=torch.uint8)
        if torch.device(dev).type == "cuda":
            self._lp_host = self._lp_host.pin_memory()
        self.top_ids, self.top_lp, self.lp = self._lp_views(self._lp_pack)
        # grounded decoding: the ids of the grammar (ValueError here when the model's do not describe it) and the per-row state
        self.grounded = bool(grounded)
        self.gids = self.gstate = self.gn = None
        if self.grounded:
            self.gids = grammar.GrammarIds.from_model(model)
            self.gstate = torch.full((max_rows,), -1, dtype=I32, device=dev)
            self.gn = torch.zeros((max_rows,), dtype=I32, device=dev)
        self.graph = self.graph_lp = self.graph_g = self.graph_lp_g = None
        self.steps = 0
        # overlapped admission: at most ONE prefill in flight (there is one staging cache), on `_side`; `_placed` orders the next
        # prefill's writes into the staging cache behind the previous batch's move into the arena
        if overlap_admission and not use_graph:
            raise ValueError("overlap_admission needs the captured decode step (use_graph=True): the eager step shares workspaces with the prefill")
        # admit_min: while rows are live, hold an admission until this many requests can go in ONE prefill (or the queue holds fewer):
        # a 1-image prefill costs 23 ms, a 4-image one 12 ms per image -- throughput for first-token latency; 1 = admit at once.  A held
        # request goes in after `admit_hold` ticks whatever has freed up (ragged traffic at 32 rows: 38.6 -> 44.9 img/s with 2,
        # profiles/r06_serve_admit_min.txt)
        self.admit_min, self.admit_hold, self._held = max(1, int(admit_min)), max(0, int(admit_hold)), 0
        self.overlap = bool(use_graph if overlap_admission is None else overlap_admission)   # default: on whenever the step is a graph
        self._job = None
        self._side = torch.cuda.Stream(device=dev) if self.overlap else None
        self._placed = None

    def _lp_views(self, buf):
        """(top_ids int64 [rows, 8], top_lp f32 [rows, 8], lp f32 [rows]) inside the log-probability buffer"""
        n = self.rows
        return buf[: n * 64].view(I64).view(n, 8), buf[n * 64: n * 96].view(F32).view(n, 8), buf[n * 96:].view(F32)

    @staticmethod
    def _check_paged(model, max_rows, max_len, grow_to, kv_pages):
        if grow_to is not None:
            raise ValueError("grow_to does not apply to a paged KV cache (its pool never moves)")
        if kv_pages < 1:
            raise ValueError("kv_pages must be >= 1")
        n_pos = int(model.config.llm_cfg.max_position_embeddings)
        if max_len % 64 or not 0 < max_len <= min(8192, n_pos):
            # (the RoPE tables have exactly max_position_embeddings rows: a position beyond them would read past the table)
            raise ValueError(f"max_len must be a multiple of 64 and <= min(8192, max_position_embeddings = {n_pos})")
        llm = model.llm
        if llm.prec is not None or llm.decode_path(max_rows, max_len) is None:
            raise ValueError("kv_pages needs a model whose decode step runs on the weight-streaming kernels (a single-type 16-bit or "
                             "e4m3 stack within the stream limits, <= 64 rows)")

    def kv_stats(self):
        """paged mode: pages total / free / high water and the bytes of the page pools and of the staging cache"""
        st = sum(t.numel() * t.element_size() for t in self.staging.k + self.staging.vt)
        if not self.paged:
            return dict(pages_total=None, pages_free=None, high_water=None,
                        pool_bytes=sum(t.numel() * t.element_size() for t in self.arena.k + self.arena.vt), staging_bytes=st)
        return dict(pages_total=self.pages.n, pages_free=self.pages.n_free, high_water=self.pages.high_water,
                    pool_bytes=self.arena.nbytes(), staging_bytes=st,
                    prefix_entries=len(self.prefix) if self.prefix is not None else 0, prefix_hits=self.prefix_hits,
                    prefix_misses=self.prefix_misses, pages_shared=self.pages.n_shared)

    def clear_prefix_cache(self):
        """drop every prefix-cache entry; pages that live rows still map stay allocated until those rows finish"""
        if self.prefix is not None:
            self.prefix.clear()

    # ------------------------------------------------------------------ admission-time warm-up
    @engine.model_entry(lambda self, *a, **kw: self.model.precision)
    def warm_admission(self, input_ids, image, rows=1):
        """One throw-away admission prefill of `rows` copies of an example request BEFORE live traffic: the hipGraphs of the ViT,
        the region pyramid and the LLaMA prefill for that batch shape are captured on this pass (engine.GraphPool.first_sight)
        instead of inside the first three live admissions of the shape, and the workspace arenas reach their working size.
        Nothing of the example survives: the staging cache is overwritten by the next admission, no slot is taken."""
        if self.slots.n_free != self.rows:
            raise RuntimeError("warm_admission() must run before the first admission")
        if self.use_graph and self.graph is None:
            self._capture()
        k = max(1, min(int(rows), self.admit_rows))
        ids = input_ids.reshape(1, -1).to(I64).cpu().repeat(k, 1)
        imgs = torch.stack([image] * k)
        def once():
            self.model.forward(input_ids=ids.clone(), images=imgs, use_cache=True, return_dict=True,
                               _cache=self.staging.rows(k), _seeds=[0] * k)
        # first pass EAGER: the workspace arenas grow to their working size and every kernel has had its first launch (lazy
        # function attributes, module load) -- a graph captured on this pass would be keyed on pre-growth addresses, never be
        # replayed, and sit in the LRU pools evicting useful ones.  Second pass: capture, on the settled addresses.
        # (overlapped admissions launch their GEMMs one workgroup per tile, ops.gemm_yield: capture that form)
        with engine.GraphPool.eager(), ops.gemm_yield(self.overlap):
            once()
        with engine.GraphPool.first_sight(), ops.gemm_yield(self.overlap):
            once()

    # ------------------------------------------------------------------ request intake
    def submit(self, input_ids, image, max_new_tokens=256, refer_boxes=None, ground_boxes=None, eos_token_id="config",
               stop_token_id=None, seed=None, temperature=0.0, logprobs=None, grounded=False):
        """grounded=True (a batcher built with grounded=True): every token obeys the region-token grammar (grammar.py) with n = the
        rows of the request's `pred_boxes`; `result(rid).grammar_state` is the state behind its last token.  The sampler runs behind
        the mask, so `logprobs` / `top_logprobs` are under the constrained distribution and alternatives past the allowed set are -inf.
        logprobs: None = off; 0 = `result(rid).logprobs` holds the natural-log probability of every returned token under softmax of
        the raw logits (temperature 1, whatever the request samples at); 1..8 = `top_logprobs` also holds, per token, that many best
        (token id, log-probability) pairs, by logit descending then id ascending."""
        if logprobs is not None and (isinstance(logprobs, bool) or int(logprobs) != logprobs or not 0 <= int(logprobs) <= 8):
            raise ValueError("logprobs must be None or an integer in 0..8")
        if grounded and not self.grounded:
            raise ValueError("submit(grounded=True) needs a batcher built with grounded=True (its grounded step is captured at construction)")
        if eos_token_id == "config":
            eos_token_id = self.model.generation_config.eos_token_id
        r = Request(self._next_rid, input_ids.reshape(-1).to(I64).cpu(), image, int(max_new_tokens), refer_boxes, ground_boxes,
                    eos_token_id, stop_token_id, seed, float(temperature), grounded=bool(grounded))
        if logprobs is not None:
            r.logprobs_k, r.logprobs = int(logprobs), []
            if r.logprobs_k:
                r.top_logprobs = []
        self._next_rid += 1
        self.queue.append(r)
        self.live[r.rid] = r
        return r.rid

    # ------------------------------------------------------------------ one decode step of every occupied row
    def _decode(self, lp=False, gr=False):
        """lp: a live row asks for log-probabilities -- the sampler is gr_sample_rows_lp (rows that do not ask: lp_k = -1); else the
        step is launch for launch what it was before that entry existed.  gr: a live row is grounded -- gr_grammar_step masks the
        logits in front of the sampler (rows that are not: gstate = -1, untouched)"""
        llm = self.llm
        ops.embed_gather(self.tok, llm.w["embed"], llm.w["new_embed"], out=self.h)
        llm.forward(self.h, self.rows, 1, self.arena, pos_dev=self.pos, pos_stride=1)
        logits = llm.decode_logits(self.rows)
        if gr:
            ops.grammar_step(logits, llm.V, self.gstate, self.gn, self.gids, last_tok=self.tok)
        self._sample(logits, lp)
        ops.greedy_advance(self.nxt, self.tok, self.occupied, self._seq, self.pos, self.step_ctr, self.n_live,
                           eos=None, pad=0, inc_pos=2)

    def _sample(self, logits, lp):
        a = dict(pos=self.pos, pos_stride=1, pos_off=1, out=self.nxt)   # greedy rows: inv_temp 0 -> arg-max
        if lp:
            ops.sample_rows_lp(logits, self.llm.V, self.inv_temp, self.seed, logprob=self.lp, k=self.lp_k, top_ids=self.top_ids,
                               top_lp=self.top_lp, **a)
        else:
            ops.sample_rows(logits, self.llm.V, self.inv_temp, self.seed, **a)

    def _capture(self):
        """Capture the step once, before any request owns a slot (the warm-up steps write KV at the idle position): `graph`, and
        `graph_lp`, the same step with the log-probability sampler, replayed on the ticks where a live row asks.  With every output off
        that kernel measured 0.25 us (1.3 %) above sample_rows_kernel at 64 rows (profiles/r09_sampler_logprobs.txt), more than the
        latter's run-to-run spread, so ticks on which nobody asks keep the plain step.  Both are captured here, never later: traffic
        that mixes requests that ask with requests that do not only chooses between them.  A batcher built with grounded=True captures
        the grounded variants of the two (`graph_g`, `graph_lp_g`) next to them, for the ticks on which a live row is grounded."""
        side = torch.cuda.Stream(device=self.tok.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self._decode()
            self._sample(self.llm.decode_logits(self.rows), True)   # (its first launch, outside a capture)
            if self.grounded:   # (likewise; no token: no state changes, and what it writes is scratch the next step overwrites)
                ops.grammar_step(self.llm.decode_logits(self.rows), self.llm.V, self.gstate, self.gn, self.gids)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs = []
        for gr in ((False, True) if self.grounded else (False,)):
            for lp in (False, True):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._decode(lp, gr)
                graphs.append(g)
        self.graph, self.graph_lp = graphs[:2]
        if self.grounded:
            self.graph_g, self.graph_lp_g = graphs[2:]

    # ------------------------------------------------------------------ KV arena growth
    def _bound(self, r):
        """upper bound of a request's context: the expanded prompt (groma.py:317-357: <image> -> the image tokens, <region> -> two ids
        per selected region, at most max_region_num + the caller's refer / ground boxes) + its new tokens"""
        m = self.model
        extra = sum(int(b.shape[0]) for b in (r.refer_boxes, r.ground_boxes) if b is not None)
        return int(r.input_ids.numel()) + (m.vit.G // 2) ** 2 + 2 * (int(m.config.max_region_num) + extra) + r.max_new_tokens

    def _grow(self, need):
        """Re-allocate the arena (and the staging cache) at max(2 x max_len, need) positions per slot, capped by grow_to.  Live rows
        keep their KV prefix (K rows / V^T columns are copied; (hi, lo) pair storage interleaves in blocks of 32, so a prefix of
        64-multiples is a prefix there too) and their loop state; the decode step is re-captured on the new addresses.
        Failure-atomic: both new caches are allocated and the prefixes copied BEFORE anything of the batcher changes; if the device
        cannot hold them (peak = old arena + old staging + both new caches) the old caches stay in service, False is returned and
        the over-long request is refused by the ordinary length checks of _admit() -- live rows are never stranded.
        Cost of a successful growth in the middle of live traffic: the copy, three eager steps + one capture, one device sync."""
        old = self.max_len
        new_len = min(self.grow_to, max(2 * old, -(-int(need) // 64) * 64))
        if new_len <= old or new_len >= getattr(self, "_grow_failed_at", 1 << 30):
            return False
        dev = self.tok.device
        try:
            staging = self.llm.new_cache(self.rows, new_len, dev)
            arena = self.llm.new_cache(self.rows, new_len, dev)
            for l in range(len(arena.k)):
                arena.k[l][:, :, :old].copy_(self.arena.k[l])
                arena.vt[l][..., : old * arena.sp].copy_(self.arena.vt[l])
        except RuntimeError as e:   # (torch.cuda.OutOfMemoryError is a RuntimeError)
            staging = arena = None
            self._grow_failed_at = new_len       # do not retry this size for every over-long request of the queue
            self.last_grow_error = str(e)
            torch.cuda.empty_cache()
            return False
        # commit: from here on nothing can fail half-way
        stale = set(engine.cache_addresses(self.staging)[1:])
        self.staging, self.arena, self.max_len = staging, arena, new_len
        # prefill graphs captured against the old staging cache can never be replayed again: free their slots in the LRU pool
        self.llm.graphs.drop(lambda key: any(a in stale for a in key))
        if self.graph is not None:
            # the three eager warm-up steps in front of a capture advance every row: keep the loop state aside and put it back (what they
            # wrote into live rows' KV lies at positions >= pos, which the next real step rewrites before it attends to them)
            keep = (self.tok, self.nxt, self.occupied, self.pos, self.step_ctr, self.n_live, self._seq, self.h)
            keep += (self.gstate,) if self.grounded else ()
            saved = [t.clone() for t in keep]
            self.graph = None
            self._capture()
            for t, v in zip(keep, saved):
                t.copy_(v)
        return True

    def _grow_for(self, reqs):
        if self.max_len < self.grow_to:
            # (_bound is a worst case -- the real spliced length is only known after the prefill -- so a request that would just
            #  have fitted can trigger a growth; the alternative, prefilling first and re-admitting, costs a second prefill)
            need = max(self._bound(r) for r in reqs)
            if need > self.max_len:
                self._grow(need)   # False: the old caches stay; the length checks of the prefill refuse what does not fit

    # ------------------------------------------------------------------ admission: one batched prefill per tick
    def _admit(self, reqs):
        """Prefill `reqs` (<= free slots) in ONE forward and move each row's KV into its slot.  Row results of the
        prefill are bit-identical to a batch-1 forward of the same request (every kernel of the path is row- /
        image-independent, tests/test_fullsize_properties_gpu.py), so admission order and company never change a
        request's tokens; each request's region shuffle draws from its own seed."""
        self._grow_for(reqs)
        self._place(reqs, self._prefill(reqs))

    def _prefill(self, reqs):
        """The device half of an admission, on the CURRENT stream: one batched forward into the staging cache + each row's first token
        (prefix-cache hits: one suffix prefill on the paged cache, _prefill_hits).  Returns [(request, staging row or None, first token,
        1/temperature)] for the requests that go on; touches neither the slot table nor the arena's table nor the loop state (with
        overlap_admission it runs on the worker thread while the decode ticks use those)."""
        cold = [r for r in reqs if r.hit is None]
        hits = [r for r in reqs if r.hit is not None]
        return (self._prefill_cold(cold) if cold else []) + (self._prefill_hits(hits) if hits else [])

    def _prefill_cold(self, reqs):
        m, k = self.model, len(reqs)
        P = max(r.input_ids.numel() for r in reqs)
        ids = torch.full((k, P), int(m.pad_token_id), dtype=I64)
        for i, r in enumerate(reqs):
            ids[i, : r.input_ids.numel()] = r.input_ids
        empty = torch.zeros((0, 4))
        rb = [r.refer_boxes if r.refer_boxes is not None else empty for r in reqs] if any(r.refer_boxes is not None for r in reqs) else None
        gb = [r.ground_boxes if r.ground_boxes is not None else empty for r in reqs] if any(r.ground_boxes is not None for r in reqs) else None
        view = self.staging.rows(k)
        try:
            out = m.forward(input_ids=ids, images=torch.stack([r.image for r in reqs]), refer_boxes=rb, ground_boxes=gb,
                            use_cache=True, return_dict=True, output_hidden_states=True, _cache=view,
                            _seeds=[r.seed for r in reqs], _keep_embeds=self.prefix is not None)
        except RuntimeError as e:
            if k == 1:
                reqs[0].done, reqs[0].error = True, str(e)
                return []
            # isolate the offender: one by one.  Each survivor's KV must be in ITS OWN staging row when the batch is placed, and a
            # batch-1 prefill lands in row 0 -- so the survivors are moved to their rows as they come
            placed = []
            for i in range(k - 1, -1, -1):   # (last to first: row 0 is where every batch-1 prefill lands, so its own request goes last)
                one = self._prefill_cold([reqs[i]])
                if one:
                    if i:
                        for l in range(len(self.staging.k)):
                            self.staging.k[l][i].copy_(self.staging.k[l][0])
                            self.staging.vt[l][i].copy_(self.staging.vt[l][0])
                    placed.append((reqs[i], i, one[0][2], one[0][3]))
            placed.reverse()
            return placed
        lengths = m._last_aux["lengths"]
        placed = []
        for i, r in enumerate(reqs):
            r.prompt_len = int(lengths[i])
            r.pred_boxes = out.hidden_states[1]["pred_boxes"][i]
            if r.prompt_len + r.max_new_tokens > self.max_len:
                r.done, r.error = True, "prompt + max_new_tokens exceeds the KV slot (max_len)"
                continue
            if self.prefix is not None:
                self._keep_prefix(r, m._last_aux["input_ids"][i, : r.prompt_len], m._last_aux["inputs_embeds"][i])
            placed.append((r, i) + self._first_token(r, out.logits[i, r.prompt_len - 1]))
        return placed

    def _first_token(self, r, logits_row):
        """(first token, 1/temperature) of a request from the logits of its last prompt position"""
        dev = self.tok.device
        it = 0.0 if r.temperature < 1e-4 else 1.0 / r.temperature
        args = (logits_row[None].contiguous(), logits_row.shape[-1], torch.tensor([it], dtype=F32, device=dev),
                torch.tensor([int(r.seed or 0)], dtype=I64, device=dev))
        pos = torch.tensor([r.prompt_len], dtype=I32, device=dev)
        if r.grounded:   # the tick's grammar step on this one row, in its start state (no token yet), on a copy of the prefill's logits
            row = ops.grammar_step(logits_row[None].clone(memory_format=torch.contiguous_format), logits_row.shape[-1],
                                   torch.zeros((1,), dtype=I32, device=dev),
                                   torch.tensor([int(r.pred_boxes.shape[0])], dtype=I32, device=dev), self.gids)
            args = (row,) + args[1:]
        if r.logprobs_k is None:
            return int(ops.sample_rows(*args, pos=pos)[0]), it
        # the first token's log-probability (and alternatives): the tick's sampler on this one row; kept on the request until _place emits it
        top_ids, top_lp = torch.full((1, 8), -1, dtype=I64, device=dev), torch.full((1, 8), float("-inf"), dtype=F32, device=dev)
        ids, lp = ops.sample_rows_lp(*args, pos=pos, k=torch.tensor([r.logprobs_k], dtype=I32, device=dev), top_ids=top_ids, top_lp=top_lp)
        r._first_lp = (float(lp[0]), top_ids[0].tolist(), top_lp[0].tolist())
        return int(ids[0]), it

    # ------------------------------------------------------------------ prefix cache
    def _keep_prefix(self, r, ids_x, emb):
        """a cold request that may become a prefix-cache entry at placement: keep its expanded ids and the LLM input rows from the page
        of its last injected (image / region) row to the end of the prompt -- the only prefix rows a later suffix prefill recomputes"""
        r._entry = None
        key = getattr(r, "_key", None)
        xs = ids_x.tolist()
        inj = [j for j, x in enumerate(xs) if x in self._inj]
        if key is None or not inj or r.prompt_len < 64 or self.model.pad_token_id in r.input_ids.tolist():
            return
        e0 = 64 * (inj[-1] // 64)
        r._entry = (key, ids_x.clone(), emb[e0: r.prompt_len].clone(), e0)

    def _match(self, r):
        """paged mode with the cache on: the request's PrefixMatch, or None (a cold admission).  A hit's suffix, padded to the wave's
        common length, must stay inside max_len (the RoPE tables): a hit that could not is run cold."""
        m = self.model
        r._key = key = prefix_key(r.image, r.seed, r.refer_boxes, r.ground_boxes,
                                  (m.precision, getattr(m, "vit_precision", None), bool(self.llm.w["fp8"])))
        if key is None:
            return None
        hit = self.prefix.match(key, r.input_ids)
        if hit is None or hit.L + r.max_new_tokens > self.max_len or hit.p0 + max(9, hit.L - hit.p0) > self.max_len:
            return None
        return hit

    def _prefill_hits(self, reqs):
        """One suffix prefill for the prefix-cache hits of a wave, on the CURRENT stream: row b prefills positions [p0_b, L_b) on the
        paged cache through the admission table (its entry's shared pages below p0_b, then its own), from the entry's stored input rows
        of [p0_b, c_b) and the embeddings of its own ids behind the shared prefix.  Rows are padded to a common length (at least 2 and
        more than 8 rows in all: the prefill GEMM forms); what a padding position writes lands in a page of its own row or in the sink
        page.  Returns the placed tuples, first tokens sampled as _prefill_cold samples them."""
        groups = []   # (a padded position must stay below max_len, the RoPE tables' bound: rare waves split, _match admits every row alone)
        for r in reqs:
            for g in groups:
                if all(x.hit.p0 + self._wave_len(g + [r]) <= self.max_len for x in g + [r]):
                    g.append(r)
                    break
            else:
                groups.append([r])
        return [p for g in groups for p in self._suffix_prefill(g)]

    @staticmethod
    def _wave_len(reqs):
        """the common suffix length of a wave: its longest suffix, at least 2 and more than 8 rows in all (the prefill GEMM forms)"""
        return max(max(r.hit.L - r.hit.p0 for r in reqs), 2, -(-9 // len(reqs)))

    def _suffix_prefill(self, reqs):
        llm, dev, T = self.llm, self.tok.device, self.llm.T
        k = len(reqs)
        Lq = self._wave_len(reqs)
        h = torch.zeros((k * Lq, T), dtype=F32, device=dev)
        tab = torch.zeros((k, self._adm_table.shape[1]), dtype=I32)
        for b, r in enumerate(reqs):
            m, e = r.hit, r.hit.entry
            r.prompt_len = m.L
            r.pred_boxes = e.pred_boxes.clone()
            h[b * Lq: b * Lq + m.c - m.p0].copy_(e.rows[m.p0 - e.e0: m.c - e.e0])
            if m.L > m.c:
                llm.embed(r.input_ids[m.u:].to(dev), out=h[b * Lq + m.c - m.p0: b * Lq + m.L - m.p0])
            tab[b, : len(r.pages)] = torch.tensor(r.pages, dtype=I32)
        self._adm_table[:k].copy_(tab)
        pos = torch.tensor([r.hit.p0 for r in reqs], dtype=I32).to(dev)
        kv_len = torch.tensor([r.hit.L for r in reqs], dtype=I32).to(dev)
        logits = llm.prefill_paged(h, k, Lq, self.arena, self._adm_table, pos, kv_len)
        return [(r, None) + self._first_token(r, logits[b, r.hit.L - 1 - r.hit.p0]) for b, r in enumerate(reqs)]

    def _place(self, reqs, placed):
        """The host half of an admission, on the decode stream between two ticks: emit the first tokens, hand out slots, move the rows'
        KV from the staging cache into the arena, arm the loop state."""
        rows, slots = [], []
        for r, i, first, it in placed:
            self._emit(r, first, r.__dict__.pop("_first_lp", None))
            if r.done:
                continue
            r.slot = self.slots.acquire(r.rid)
            rows.append(i)
            slots.append(r.slot)
            self.tok[r.slot] = first
            self.pos[r.slot] = r.prompt_len
            self.occupied[r.slot] = 1
            self.inv_temp[r.slot] = it
            self.seed[r.slot] = int(r.seed or 0)
            self.lp_k[r.slot] = -1 if r.logprobs_k is None else r.logprobs_k
            if self.grounded:   # TEXT: the tick's kernel moves it on by `first`
                self.gstate[r.slot] = 0 if r.grounded else -1
                self.gn[r.slot] = int(r.pred_boxes.shape[0]) if r.grounded else 0
        if self.paged:
            self._place_pages(reqs, placed, rows)
            return
        if rows:
            dev = self.tok.device
            src = torch.tensor(rows, dtype=I64, device=dev)
            dst = torch.tensor(slots, dtype=I64, device=dev)
            # only the prefix the prompts fill (whole 64-position blocks: a prefix in the pair layout too): what lies behind a row's
            # position is rewritten by its own decode steps before it is ever attended to
            n = min(self.max_len, -(-max(r.prompt_len for r, _, _, _ in placed if r.slot is not None) // 64) * 64)
            sp = self.arena.sp
            for l in range(len(self.arena.k)):
                self.arena.k[l][:, :, :n].index_copy_(0, dst, self.staging.k[l][:, :, :n].index_select(0, src))
                self.arena.vt[l][..., : n * sp].index_copy_(0, dst, self.staging.vt[l][..., : n * sp].index_select(0, src))

    def _place_pages(self, reqs, placed, rows):
        """paged mode, on the decode stream: keep the pages a placed request's prompt + new tokens can reach, give back the rest (and
        all of them for a request that did not go on), write the rows' block-table entries and move their prompt KV into the pages"""
        for r in reqs:
            if r.slot is None:
                if r.pages:
                    self.pages.release(r.pages)
                r.pages, r._entry = None, None
                continue
            keep = -(-(r.prompt_len + r.max_new_tokens) // 64)
            if keep < len(r.pages):
                self.pages.release(r.pages[keep:])
                r.pages = r.pages[:keep]
        live = [r for r, _, _, _ in placed if r.slot is not None]
        if not live:
            return
        dev = self.tok.device
        tab = torch.zeros((len(live), self.arena.table.shape[1]), dtype=I32)
        for j, r in enumerate(live):
            tab[j, : len(r.pages)] = torch.tensor(r.pages, dtype=I32)
        slots = torch.tensor([r.slot for r in live], dtype=I64, device=dev)
        self.arena.table.index_copy_(0, slots, tab.to(dev))
        # prefix-cache hits prefilled straight into their pages: only the cold rows come from the staging cache
        cold = [(r, i) for r, i, _, _ in placed if r.slot is not None and i is not None]
        if not cold:
            return
        meta = torch.tensor([[i for _, i in cold], [r.slot for r, _ in cold], [r.prompt_len for r, _ in cold]], dtype=I32).to(dev)
        n = max(r.prompt_len for r, _ in cold)
        for l in range(len(self.arena.k)):
            ops.kv_scatter_pages(self.staging.k[l], self.staging.vt[l], self.arena.k[l], self.arena.vt[l], self.arena.table, meta,
                                 min(n, self.max_prompt_len))
        if self.prefix is not None:   # a cold prompt's whole pages become an entry
            for r, _ in cold:
                kept = getattr(r, "_entry", None)
                r._entry = None
                if kept is not None:
                    key, ids_x, rows, e0 = kept
                    self.prefix.add(key, r.input_ids, ids_x, r.pred_boxes.clone(), r.pages[: r.prompt_len // 64], rows, e0)

    def _take_batch(self):
        """the requests of the next admission wave, off the head of the queue.  Slot mode: as many as there are free slots.  Paged mode:
        FIFO while a row is free and the head request's ceil(bound / 64) pages are (reserved here, at the decision); a request that can
        never fit finishes with `error`, one that does not fit yet waits at the head.  Returns (batch, refused)."""
        if not self.paged:
            return [self.queue.popleft() for _ in range(min(len(self.queue), self.slots.n_free))], []
        batch, refused = [], []
        while self.queue and len(batch) < min(self.slots.n_free, self.admit_rows):
            r = self.queue[0]
            bound = self._bound(r)
            need = -(-bound // 64)
            err = None
            if bound > self.max_len:
                err = f"the request's context bound {bound} exceeds max_len {self.max_len}"
            elif need > self.pages.n:
                err = f"the request's context bound {bound} needs {need} pages, more than the pool's {self.pages.n}"
            elif bound - r.max_new_tokens > self.max_prompt_len:
                err = f"the request's prompt bound {bound - r.max_new_tokens} exceeds max_prompt_len {self.max_prompt_len}"
            if err is not None:
                self.queue.popleft()
                r.done, r.error = True, err
                refused.append(r)
                continue
            if self.prefix is not None:
                ids = self._reserve_prefixed(r, need)
            else:
                ids = self.pages.reserve(need)
            if ids is None:
                break
            self.queue.popleft()
            r.pages = ids
            batch.append(r)
        return batch, refused

    def _reserve_prefixed(self, r, need):
        """prefix cache on: the request's pages -- a hit maps its entry's pages below p0 (one more holder each) and reserves the rest of
        its exact context; a miss reserves `need` as without the cache.  Least recently used entries are evicted while a reservation
        cannot be met.  None (nothing held) when it cannot be met without them either."""
        hit = self._match(r)
        shared = hit.entry.pages[: hit.p0 // 64] if hit is not None else []
        if hit is not None:
            self.pages.retain(shared)   # (before any eviction: the entry may be the one evicted)
            self.prefix.touch(hit.entry)
            need = -(-(hit.L + r.max_new_tokens) // 64) - len(shared)
        ids = self.pages.reserve(need)
        while ids is None and self.prefix.evict():
            ids = self.pages.reserve(need)
        if ids is None:
            if shared:
                self.pages.release(shared)
            return None
        r.hit = hit
        if hit is not None:
            self.prefix_hits += 1
        else:
            self.prefix_misses += 1
        return shared + ids

    # ------------------------------------------------------------------ overlapped admission (worker thread + side stream)
    def _launch_admission(self, reqs):
        """start the prefill of `reqs` on the worker thread; the caller has made sure no other one is in flight"""
        job = {"reqs": reqs, "placed": [], "done": threading.Event(), "event": None, "error": None}
        if self._placed is not None:
            self._side.wait_event(self._placed)   # the previous batch has left the staging cache
        else:
            self._side.wait_stream(torch.cuda.current_stream())
        if any(r.hit is not None for r in reqs):
            # a suffix prefill writes pages straight away: behind the decode stream's last table update (pages freed by rows that
            # finished since) and every placement that filled the pages it maps
            self._side.wait_stream(torch.cuda.current_stream())

        job["thread"] = threading.Thread(target=self._admission_work, args=(job,), name="groma-admission", daemon=True)
        self._job = job
        job["thread"].start()

    @engine.model_entry(lambda self, *a, **kw: self.model.precision)
    def _admission_work(self, job):
        """worker thread: the operand type, no-grad mode, current stream and GEMM grid form are all per thread"""
        try:
            with torch.cuda.stream(self._side), ops.gemm_yield():   # (one workgroup per GEMM tile: the ticks' kernels get CUs as tiles retire)
                job["placed"] = self._prefill(job["reqs"])
                ev = torch.cuda.Event()
                ev.record(self._side)
                job["event"] = ev
        except BaseException as e:   # never leave the batcher waiting for a job that died
            job["error"] = e
        finally:
            job["done"].set()

    def _finish_admission(self, wait=False):
        """place the rows of a finished prefill (wait=True: block until it has finished).  Returns the admission events."""
        job = self._job
        if job is None or not (wait or job["done"].is_set()):
            return []
        job["done"].wait()
        job["thread"].join()
        self._job = None
        if job["error"] is not None:
            for r in job["reqs"]:
                if not r.done:
                    r.done, r.error = True, f"admission failed: {job['error']}"
                if r.pages:   # (paged mode: nothing of the wave was placed)
                    self.pages.release(r.pages)
                    r.pages = None
            if not isinstance(job["error"], Exception):
                raise job["error"]
        else:
            torch.cuda.current_stream().wait_event(job["event"])
            self._place(job["reqs"], job["placed"])
            self._placed = torch.cuda.Event()
            self._placed.record(torch.cuda.current_stream())
        return [(r.rid, r.tokens[-1] if r.tokens else None, r.done) for r in job["reqs"]]

    def _emit(self, r, token, lp=None):
        """lp: (log-probability, the 8 top ids, the 8 top log-probabilities) of `token`, for a request that asked"""
        r.tokens.append(token)
        if r.logprobs_k is not None:
            r.logprobs.append(lp[0])
            if r.logprobs_k:
                r.top_logprobs.append(list(zip(lp[1][: r.logprobs_k], lp[2][: r.logprobs_k])))
        if (r.eos_token_id is not None and token == r.eos_token_id) or \
                (r.stop_token_id is not None and token == r.stop_token_id) or len(r.tokens) >= r.max_new_tokens:
            self._finish(r)

    def _finish(self, r):
        r.done = True
        if r.grounded:
            r.grammar_state = grammar.final_state(r.tokens, self.gids)
        if r.slot is not None:
            s = r.slot
            self.occupied[s] = 0
            self.pos[s] = 0
            self.lp_k[s] = -1
            if self.grounded:
                self.gstate[s] = -1
            if self.paged:
                # the row's entries point at the sink page again (on the decode stream, so before any later _place can
                # write these pages into another row's entries), then the pages go back to the pool
                self.arena.table[s].zero_()
                self.pages.release(r.pages)
                r.pages = None
            self.slots.release(s)
            r.slot = None

    # ------------------------------------------------------------------ scheduler tick
    @engine.model_entry(lambda self, *a, **kw: self.model.precision)
    def step(self):
        """Admit what fits, then advance every occupied row by one token.  Returns [(rid, token, done), ...]."""
        if self.use_graph and self.graph is None:
            if self.slots.n_free != self.rows:
                raise RuntimeError("capture must precede the first admission")
            self._capture()
        events = []
        if self.overlap:
            events += self._finish_admission()
            if self._job is None and self._may_admit():
                batch, refused = self._take_batch()
                events += [(r.rid, None, True) for r in refused]
                if batch:
                    self._grow_for(batch)
                    self._launch_admission(batch)
            if self._job is not None and not self.slots.active():
                events += self._finish_admission(wait=True)   # nothing to decode meanwhile: wait for the rows
        elif self._may_admit():
            batch, refused = self._take_batch()
            events += [(r.rid, None, True) for r in refused]
            if batch:
                self._admit(batch)
            for r in batch:
                events.append((r.rid, r.tokens[-1] if r.tokens else None, r.done))
        act = self.slots.active()
        if not act:
            return events
        # a tick on which a live row asked for log-probabilities runs the step with that sampler and queues ONE more copy
        # (asynchronous, into pinned memory) in front of the ids' read, whose synchronisation covers it
        ask = any(self.live[self.slots.owner[s]].logprobs_k is not None for s in act)
        gr = self.grounded and any(self.live[self.slots.owner[s]].grounded for s in act)
        if self.use_graph:
            if gr:
                (self.graph_lp_g if ask else self.graph_g).replay()
            else:
                (self.graph_lp if ask else self.graph).replay()
        else:
            self._decode(ask, gr)
        self.steps += 1
        if ask:
            self._lp_host.copy_(self._lp_pack, non_blocking=True)
        new = self.tok.tolist()  # the only per-step synchronisation: max_rows ids
        if ask:
            top_ids, top_lp, lps = (t.tolist() for t in self._lp_views(self._lp_host))
        for s in act:
            r = self.live[self.slots.owner[s]]
            self._emit(r, int(new[s]), (lps[s], top_ids[s], top_lp[s]) if r.logprobs_k is not None else None)
            events.append((r.rid, r.tokens[-1], r.done))
        return events

    def _may_admit(self):
        n = min(len(self.queue), self.slots.n_free)
        if n == 0:
            return False
        if n >= min(self.admit_min, len(self.queue)) or self.slots.n_free == self.rows or self._held >= self.admit_hold:
            self._held = 0
            return True
        self._held += 1
        return False

    def run_until_done(self, max_steps=100000):
        for _ in range(max_steps):
            if not self.queue and not self.slots.active() and self._job is None:
                break
            self.step()
        return {rid: r for rid, r in self.live.items()}

    def result(self, rid, pop=True):
        r = self.live.pop(rid) if pop else self.live[rid]
        return r

    # ------------------------------------------------------------------ model_worker.generate_stream analogue
    def generate_stream(self, input_ids, image, max_new_tokens=256, stream_interval=1, **kw):
        """Yield the generated ids of ONE request every `stream_interval` tokens while other requests keep decoding
        (groma/serve/model_worker.py:287-338 yields the decoded text; tokenisation stays with the caller).  Keywords go to submit()
        (grounded=True: the yielded ids obey the region-token grammar).  With logprobs=k (see
        submit) every yield is (ids, logprobs, top_logprobs) instead, the lists aligned one to one (top_logprobs None for k = 0)."""
        rid = self.submit(input_ids, image, max_new_tokens=max_new_tokens, **kw)
        r = self.live[rid]
        sent = 0
        while not r.done:
            self.step()
            if r.error:
                raise RuntimeError(r.error)
            if len(r.tokens) - sent >= stream_interval or r.done:
                sent = len(r.tokens)
                if r.logprobs_k is None:
                    yield list(r.tokens)
                else:
                    yield list(r.tokens), list(r.logprobs), (list(r.top_logprobs) if r.logprobs_k else None)
        self.live.pop(rid, None)
