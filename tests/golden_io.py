"""Helpers to load the committed golden vectors and regenerate their weights."""
import os

import numpy as np

from prodiff_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


PART_BYTES = 900 * 1024      # array bytes per file: every committed fixture file stays under 1 MiB


def part_paths(name, root=GOLDEN):
    """name.npz, then name.p1.npz, name.p2.npz, ... as far as they exist."""
    paths, i = [os.path.join(root, name + ".npz")], 1
    while os.path.exists(os.path.join(root, f"{name}.p{i}.npz")):
        paths.append(os.path.join(root, f"{name}.p{i}.npz"))
        i += 1
    return paths


def save(name, arrays, root=GOLDEN, part_bytes=PART_BYTES):
    """Write a fixture as name.npz and, where its arrays exceed part_bytes, name.p1.npz, ...: arrays
    fill the parts in order; one larger than a part is cut along its flattened length into
    key@0, key@1, ... beside key@shape.  load() puts them together again.  Returns the paths."""
    parts, room = [{}], part_bytes

    def put(k, v):
        nonlocal room
        if v.nbytes > room and parts[-1]:
            parts.append({})
            room = part_bytes
        parts[-1][k] = v
        room -= v.nbytes

    for k, v in arrays.items():
        v = np.asarray(v)
        assert "@" not in k, k
        if v.nbytes <= part_bytes:
            put(k, v)
            continue
        flat, n = v.reshape(-1), max(1, part_bytes // v.itemsize)
        put(k + "@shape", np.array(v.shape, np.int64))
        for i in range(0, flat.size, n):
            put(f"{k}@{i // n}", flat[i:i + n])
    for old in part_paths(name, root)[1:]:
        os.remove(old)
    paths = []
    for i, p in enumerate(parts):
        paths.append(os.path.join(root, name + (f".p{i}" if i else "") + ".npz"))
        np.savez_compressed(paths[-1], **p)
    return paths


def load(name, root=GOLDEN):
    d = {}
    for path in part_paths(name, root):
        with np.load(path) as z:
            d.update({k: z[k] for k in z.files})
    for key in [k for k in d if k.endswith("@shape")]:
        k = key[:-len("@shape")]
        shape, chunks, i = d.pop(key), [], 0
        while f"{k}@{i}" in d:
            chunks.append(d.pop(f"{k}@{i}"))
            i += 1
        d[k] = np.concatenate(chunks).reshape([int(s) for s in shape])
    return d


def wavenet_params(dims, seed):
    M, H, L, C, _ = [int(v) for v in dims]
    return synth.synth_params(synth.wavenet_param_shapes(M, H, L, C), int(seed))


def fastdiff_params(seed):
    return synth.synth_params(synth.fastdiff_param_shapes(), int(seed))


PRODIFF_SEEDS = {"prodiff_t2_m80": (80, 21), "prodiff_t4_m80": (80, 22), "prodiff_t4_m128": (128, 23)}


def prodiff_params(name):
    M, seed = PRODIFF_SEEDS[name]
    return synth.synth_params(synth.wavenet_param_shapes(M, 256, 20, 256), seed)


def prodiff_buffers(d):
    return {k[4:]: v for k, v in d.items() if k.startswith("buf_")}


COND_INPUTS = ("lang_seq", "spk_embed_id", "spk_mix_embed", "gender_embed_id", "voicing", "breath")


def cond_case(name):
    """(hparams, params, inputs, golden) of a tests/golden/cond_*.npz fixture (gen_golden.gen_cond)."""
    d = load(name)
    over = {str(k): int(v) for k, v in zip(d["hp_keys"], d["hp_vals"])}
    hp = dict(synth.COND_DEFAULTS)
    hp.update(over)
    if int(d.get("grow", 0)):   # the reference's RelPositionalEncoding table had grown to this many rows
        hp["rel_pos_len"] = int(d["grow"])
    P = synth.synth_cond_params(synth.cond_param_shapes(int(d["vocab"]), **hp), int(d["param_seed"]))
    ins = {k: d[k] for k in ("txt_tokens", "mel2ph", "f0") + COND_INPUTS if k in d}
    if str(d["spk_mode"]) != "id":
        ins.pop("spk_embed_id")
    if not hp["use_voicing_embed"]:
        ins.pop("voicing", None)
    if not hp["use_breath_embed"]:
        ins.pop("breath", None)
    return hp, P, ins, d


COND_CASES = ("cond_small", "cond_handler", "cond_mix_gender", "cond_long", "cond_relpos", "cond_relpos_grown")
