"""Doubles for the host tests of language identification (tests/test_language_host.py): a scripted recording of three strided
windows, a pipeline around an engine double, and shards that capture / replay the rank gather.  Host-only: no GPU."""
import numpy as np

from crisperwhisper_amd import collate, dist
from crisperwhisper_amd.pipeline import CrisperWhisperPipeline

PCM = np.zeros(55 * 16000, np.float32)                       # windows at 0, 20 and 40 s
STRIDES = [(30.0, 0.0, 5.0), (30.0, 5.0, 5.0), (15.0, 5.0, 0.0)]
LANGS = ("en", "de", "es")                                   # what the scripted seek loop "detects" in window 0, 1, 2


def window(v, segments):
    """One window's tokens: for every (words, t0, t1) <|t0|> words... <|t1|> over the byte vocabulary, token timestamps spread
    over each segment."""
    tb = v.timestamp_begin
    toks, ts = [], []
    for words, t0, t1 in segments:
        seg = [tb + int(round(t0 / 0.02))] + [b for w in words for b in (" " + w).encode()] + [tb + int(round(t1 / 0.02))]
        toks += seg
        ts += np.linspace(t0, t1, len(seg)).tolist()
    return np.asarray(toks, np.int64), np.asarray(ts, np.float32)


def script(v):
    """Three 30 s windows of one recording.  Every window closes a segment of its own well inside itself (so its words are
    flushed under its own language) and the texts overlap at the seams (so tokens are dropped by the seam merge).  Per window
    (tokens, token timestamps, log-probabilities, masses, spreads); the per-token values name their token by its global index:
    logprob = -(1 + i), mass = 1 / (2 + i), spread = 0.001 * (1 + i)."""
    spans = [[(["ab", "cd"], 0.0, 8.0), (["ef", "gh"], 9.0, 29.0)],
             [(["ef", "gh"], 1.0, 9.0), (["ij", "kl"], 10.0, 20.0)],
             [(["ij", "kl"], 1.0, 6.0), (["mn", "op"], 7.0, 14.0)]]
    out, n0 = [], 0
    for segs in spans:
        tok, ts = window(v, segs)
        i = n0 + np.arange(len(tok))
        out.append((tok, ts, (-(1.0 + i)).astype(np.float32), (1.0 / (2 + i)).astype(np.float32), (0.001 * (1 + i)).astype(np.float32)))
        n0 += len(tok)
    return out


class LangScriptedEngine:
    """Window k of the recording decodes to script(v)[k] in language LANGS[k].  ``mel`` is handed the clips of one batch; the
    windows they are come from ``order`` (the windows this rank runs, in order)."""

    def __init__(self, spec, v, order):
        self.spec, self.v, self.order, self.max_batch, self.batch = spec, v, list(order), 8, []
        self.alignment_scores_on = False
        self.script = script(v)
        self.k = 0

    def mel(self, clips):
        self.batch = [self.order.pop(0) for _ in clips]
        return None, np.asarray([min(3000, len(c) // 160) for c in clips])

    def transcribe(self, nb, num_frames, **kw):
        assert nb == len(self.batch) and kw["language_token"] == -1 and len(kw["lang_ids"]) == 4
        return [self.script[k][0] for k in self.batch], [self.script[k][1] for k in self.batch], 1

    def transcribe_languages(self, B):
        assert B == len(self.batch)
        return (np.asarray([self.v.lang_id(LANGS[k]) for k in self.batch], np.int32), np.full(B, 0.75, np.float32))

    def set_token_logprobs(self, on):
        pass

    def set_top_logprobs(self, k):
        self.k = k

    def set_alignment_scores(self, on, collar_frames=0):
        self.alignment_scores_on = bool(on)

    def transcribe_token_logprobs(self, lens):
        return [self.script[k][2] for k in self.batch]

    def transcribe_top_logprobs(self, lens):
        return ([np.stack([np.arange(self.k, dtype=np.int32) + 65] * len(self.script[k][2])) for k in self.batch],
                [np.stack([self.script[k][2] - j for j in range(self.k)], axis=1) for k in self.batch])

    def transcribe_alignment_scores(self, lens):
        return [self.script[k][3] for k in self.batch], [self.script[k][4] for k in self.batch]


def make_pipe(spec, v, eng, shard=None, batch_size=1):
    """A pipeline object around an engine double: the attributes ``__call__`` reads, without a device."""
    p = object.__new__(CrisperWhisperPipeline)
    p.bundle = type("B", (), {"spec": spec})()
    p.vocab = collate.Vocabulary.from_synthetic(v)
    p.tokenizer = p.vocab
    p.sampling_rate = 16000
    p.engine, p.engines = eng, [eng]
    p.shard = shard or dist.Shard()
    p.batch_size, p.max_rows = batch_size, 8
    p.chunk_length_s, p.stride_length_s = 30, 5
    p.return_timestamps, p.return_scores, p.top_logprobs = "word", False, 0
    p.default_num_beams, p.sampling_seed, p.stats = 5, None, {}
    return p


class Captured(Exception):
    pass


class CaptureShard(dist.Shard):
    """Rank ``rank`` of ``world``: keeps what it would send and stops the call there."""

    def all_gather_records(self, recs, max_per_rank):
        self.sent, self.max_per_rank = recs, max_per_rank
        raise Captured


class ReplayShard(dist.Shard):
    """Rank 0 of ``world``: the gather returns what every rank sent, padded and ordered as the collective does."""

    def __init__(self, sent, world):
        super().__init__(0, world)
        self.all_sent = sent

    def all_gather_records(self, recs, max_per_rank):
        assert recs.tobytes() == self.all_sent[0].tobytes()
        width = recs.shape[1]
        bufs = []
        for s in self.all_sent:
            assert s.shape[1] == width                        # an empty shard sends the width the others send
            buf = np.full((max_per_rank, width), -1, np.int32)
            buf[:len(s)] = s
            bufs.append(buf)
        allr = np.concatenate(bufs)
        allr = allr[allr[:, 0] >= 0]
        return allr[np.argsort(allr[:, 0], kind="stable")]
