"""Alignment-head selection for a Whisper checkpoint: runs the forced alignment of timestamped data separately for every decoder
cross-attention head (CrisperWhisperPipeline.rank_alignment_heads) and prints the ranking and the `alignment_heads` line for the
checkpoint's generation_config.json.

The manifest is JSON lines: {"audio": path, "words": [{"text": ..., "start": seconds, "end": seconds}, ...]}, audio of at most
30 s.  The transcript of a line is its words joined by spaces; the tokenizer's word split must give the same number of words.
The checkpoint needs no alignment heads of its own: it is loaded with a placeholder.

usage: python tools/select_alignment_heads.py --model DIR --manifest FILE.jsonl [--top 15] [--collar 0.05] [--dtype bf16]
                                              [--language en] [--batch-size 8]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_manifest(path):
    base = os.path.dirname(os.path.abspath(path))
    audio, texts, refs = [], [], []
    for n, line in enumerate(open(path), 1):
        if not line.strip():
            continue
        row = json.loads(line)
        if "audio" not in row or not row.get("words"):
            raise ValueError(f"{path}:{n}: a line is {{\"audio\": path, \"words\": [{{\"text\", \"start\", \"end\"}}, ...]}}")
        for w in row["words"]:
            if not all(k in w for k in ("text", "start", "end")):
                raise ValueError(f"{path}:{n}: word {w!r} needs text, start and end")
        a = row["audio"]
        audio.append(a if os.path.isabs(a) else os.path.join(base, a))
        texts.append(" " + " ".join(w["text"].strip() for w in row["words"]))
        refs.append([{"text": w["text"], "timestamp": (float(w["start"]), float(w["end"]))} for w in row["words"]])
    if not audio:
        raise ValueError(f"{path}: no lines")
    return audio, texts, refs


def make_pipeline(a):
    import crisperwhisper_amd as cw
    from transformers import WhisperTokenizer
    bundle = cw.ModelBundle.from_pretrained(a.model, alignment_heads=[[0, 0]])     # placeholder: every head is measured
    return cw.pipeline("automatic-speech-recognition", model=bundle, tokenizer=WhisperTokenizer.from_pretrained(a.model),
                       batch_size=a.batch_size, num_beams=1, return_timestamps="word", torch_dtype=a.dtype, device="cuda:0")


def format_table(result):
    lines = ["rank  layer  head  within_collar  mean_iou  mean_abs_error_s  mean_similarity"]
    for r, row in enumerate(result["ranking"], 1):
        lines.append(f"{r:4d}  {row['head'][0]:5d}  {row['head'][1]:4d}  {row['within_collar']:13.4f}  {row['mean_iou']:8.4f}  "
                     f"{row['mean_abs_error']:16.4f}  {row['mean_similarity']:15.4f}")
    return "\n".join(lines)


def main(argv=None, make_pipeline=make_pipeline, out=sys.stdout):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True); ap.add_argument("--manifest", required=True)
    ap.add_argument("--top", type=int, default=15); ap.add_argument("--collar", type=float, default=0.05)
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--language", default=None)
    ap.add_argument("--batch-size", type=int, default=8)
    a = ap.parse_args(argv)
    audio, texts, refs = read_manifest(a.manifest)
    pipe = make_pipeline(a)
    lang = a.language if a.language is None or a.language.startswith("<|") else f"<|{a.language}|>"
    result = pipe.rank_alignment_heads(audio, texts, refs, top=a.top, collar=a.collar, language=lang, task="transcribe")
    print(format_table(result), file=out)
    print('"alignment_heads": ' + json.dumps(result["alignment_heads"]), file=out)
    return result


if __name__ == "__main__":
    main()
