"""Image retrieval on the device: a global descriptor per image aggregated from its 128-D local descriptors, a vocabulary
trained on them, and the top ``num_matched`` database images per query, so that the lists ``formats.match_pairs``,
``mapper.reconstruct`` (``pairs``) and ``retrieval.localize_by_retrieval`` (``retrieval``) start from need no outside file.

Nothing here restates the reference, which ships no retrieval network and reads the lists hloc's NetVLAD wrote.  The descriptor
is plain VLAD (Jegou et al.) with intra-normalisation (Arandjelovic and Zisserman); the pair list follows the conventions of
hloc's pairs_from_retrieval as remembered (self excluded, ``num_matched`` per image).  Parity with either is not claimed.

The kernels are csrc/imgret.hip: nearest centre per descriptor and the residual sums in float64 with every sum in
a fixed order, the two normalisations, and an exact-fp32 MFMA product whose top-k never writes the queries x database matrix.
torch here is plumbing: uploads, the walk over the images in chunks of ``image_chunk`` (the float64 sums are a workspace of the
chunk, not of the map; the result does not depend on the chunk) and the read-back of a list.

A vocabulary belongs to a descriptor type and should come from a broader sample than the map it indexes: VLAD encodes an image
relative to the vocabulary and discriminates nothing among images that all show the very points the vocabulary was trained on
(their residual sums nearly cancel)."""
from __future__ import annotations

from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from pram_amd import ops
from pram_amd._lib import PramHipError

DIM = ops.IMGRET_DIM
VOCAB_BLOCK = 1024      # rows per block of the Lloyd step's sums: the vocabulary's bits depend on it
_U = np.uint64


def _device(device) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise PramHipError("image_retrieval: expected a CUDA device (pram_amd has no CPU path)")
    return device


def _sm64(x):
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=_U) + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
        return x ^ (x >> _U(31))


def initial_rows(n: int, k: int, seed: int) -> np.ndarray:
    """k distinct rows below n by the library's sampler recipe (include/pram_hip.h at pram_pose_hypotheses): key = sm64(sm64(seed)),
    pick j = mulhi64(sm64(key + j), n - j), stepped over the earlier picks in ascending order."""
    if not 1 <= k <= n:
        raise ValueError(f"initial_rows: needs 1 <= k <= n, got k = {k}, n = {n}")
    key = int(_sm64(_sm64(np.array([seed & 0xFFFFFFFFFFFFFFFF], dtype=_U)))[0])
    with np.errstate(over="ignore"):
        words = _sm64(np.arange(k, dtype=_U) + _U(key))      # key + j wraps like the uint64 it is
    picks, earlier = [], []
    for j in range(k):
        i = (int(words[j]) * (n - j)) >> 64
        for e in earlier:      # ascending
            i += i >= e
        picks.append(i)
        earlier = sorted(earlier + [i])
    return np.array(picks, dtype=np.int64)


class Vocabulary:
    """``centres``: float32 [k, 128] on the device."""

    def __init__(self, centres: torch.Tensor):
        if centres.dim() != 2 or centres.shape[1] != DIM or centres.dtype != torch.float32 or not 1 <= centres.shape[0] <= ops.IMGRET_MAX_K:
            raise ValueError(f"Vocabulary: expected float32 [k, {DIM}] centres with 1 <= k <= {ops.IMGRET_MAX_K}, got {tuple(centres.shape)} {centres.dtype}")
        _device(centres.device)
        self.centres = centres.contiguous()

    @property
    def k(self) -> int:
        return int(self.centres.shape[0])

    def save(self, path) -> None:
        np.savez(Path(path), centres=self.centres.cpu().numpy())

    @classmethod
    def load(cls, path, device="cuda") -> "Vocabulary":
        device = _device(device)
        with np.load(Path(path)) as z:
            return cls(torch.from_numpy(np.ascontiguousarray(z["centres"], dtype=np.float32)).to(device))


def _rows(descriptors, device) -> torch.Tensor:
    t = descriptors if torch.is_tensor(descriptors) else torch.from_numpy(np.ascontiguousarray(np.asarray(descriptors, dtype=np.float32)))
    if t.dim() != 2 or t.shape[1] != DIM:
        raise ValueError(f"expected [n, {DIM}] descriptors, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def train_vocabulary(descriptors, k: int = 64, iters: int = 20, seed: int = 0, device="cuda") -> Vocabulary:
    """descriptors [n, 128] (numpy or torch) -> a vocabulary of k centres: ``initial_rows`` picks the first centres, then ``iters``
    Lloyd iterations, no early stop: assign the rows, take the residual sums over blocks of VOCAB_BLOCK consecutive rows, add the
    blocks in ascending order, c <- float(double(c) + sum / count); a centre without a row keeps its value.  The same bits on
    every run."""
    device = _device(device)
    k, iters = int(k), int(iters)
    if not 1 <= k <= ops.IMGRET_MAX_K or iters < 0:
        raise ValueError(f"train_vocabulary: needs 1 <= k <= {ops.IMGRET_MAX_K} and iters >= 0")
    x = _rows(descriptors, device)
    n = int(x.shape[0])
    centres = x[torch.from_numpy(initial_rows(n, k, int(seed))).to(device)].contiguous()
    first_h = np.arange(0, n, VOCAB_BLOCK, dtype=np.int32)
    first = torch.from_numpy(first_h).to(device)
    count = torch.from_numpy(np.minimum(VOCAB_BLOCK, n - first_h).astype(np.int32)).to(device)
    chunk = max(1, (256 << 20) // (k * DIM * 8))      # blocks per call: the float64 sums of a chunk stay under 256 MB
    total = torch.empty(k, DIM, device=device, dtype=torch.float64)
    total_n = torch.empty(k, device=device, dtype=torch.int32)
    for _ in range(iters):
        labels, _dist = ops.imgret_assign(x, centres)
        total.zero_(), total_n.zero_()
        for a in range(0, len(first_h), chunk):
            sums, n_assigned = ops.imgret_aggregate(x, labels, centres, first[a:a + chunk], count[a:a + chunk])
            ops.imgret_fold(sums, n_assigned, total, total_n)
        ops.imgret_update(centres, total, total_n)
    return Vocabulary(centres)


def _image_rows(src, device) -> Tuple[torch.Tensor, np.ndarray, np.ndarray]:
    """(rows float32 [n_rows, 128] on the device, first, count) of the three forms global_descriptors takes."""
    if isinstance(src, dict) and "counts" in src:      # the batched extractor output: padded rows, counts
        d = src["descriptors"]
        if d.dim() != 3 or d.shape[2] != DIM:
            raise ValueError(f"features: expected descriptors [B, N, {DIM}], got {tuple(d.shape)}")
        B, N = int(d.shape[0]), int(d.shape[1])
        counts = np.clip(src["counts"].cpu().numpy().astype(np.int64).reshape(B), 0, N)
        return d.to(device=device, dtype=torch.float32).contiguous().view(B * N, DIM), (np.arange(B, dtype=np.int64) * N), counts
    if hasattr(src, "frame_off") and hasattr(src, "tables"):      # a store: the flat layout
        off = np.asarray(src.frame_off, dtype=np.int64)
        return src.tables(device)["descriptors"], off[:-1], np.diff(off)
    lens = np.array([int(np.asarray(f["descriptors"]).shape[0]) for f in src], dtype=np.int64)
    parts = [np.asarray(f["descriptors"], dtype=np.float32).reshape(-1, DIM) for f, n in zip(src, lens) if n]
    flat = np.concatenate(parts) if parts else np.zeros((1, DIM), dtype=np.float32)
    off = np.concatenate([[0], np.cumsum(lens)])
    return torch.from_numpy(flat).to(device), off[:-1], lens


@torch.no_grad()
def global_descriptors(vocab: Vocabulary, frames_or_features, image_chunk: int = 1024) -> torch.Tensor:
    """One VLAD vector per image, float32 [n, k * 128] on the device, unit length (all zeros for an image without rows).  Takes a
    sequence of frame dicts with ``descriptors`` [n, 128], a store (``descriptors`` with ``frame_off``) or the batched extractor
    output (``descriptors`` [B, N, 128] with ``counts``: the rows behind a count never reach a sum)."""
    image_chunk = int(image_chunk)
    if image_chunk < 1:
        raise ValueError("image_chunk: an integer >= 1")
    dev = vocab.centres.device
    rows, first_h, count_h = _image_rows(frames_or_features, dev)
    if int(rows.shape[0]) >= 2 ** 31 or (len(first_h) and int((first_h + count_h).max()) > int(rows.shape[0])):
        raise ValueError("global_descriptors: the images' row ranges do not fit the descriptors")
    n_img, k = len(first_h), vocab.k
    out = torch.empty(max(n_img, 1), k * DIM, device=dev, dtype=torch.float32)
    if n_img == 0:
        return out[:0]
    first = torch.from_numpy(first_h.astype(np.int32)).to(dev)
    count = torch.from_numpy(count_h.astype(np.int32)).to(dev)
    labels, _dist = ops.imgret_assign(rows, vocab.centres)
    for a in range(0, n_img, image_chunk):
        b = min(a + image_chunk, n_img)
        sums, _n = ops.imgret_aggregate(rows, labels, vocab.centres, first[a:b], count[a:b])
        ops.imgret_normalize(sums, out=out[a:b])
    return out


def default_splits(nq: int, nd: int) -> int:
    """Database ranges per query tile: enough workgroups for two per compute unit of a 256-unit device, at most one per tile."""
    q_tiles = max(1, -(-int(nq) // ops.IMGRET_QUERY_TILE))
    d_tiles = max(1, -(-int(nd) // ops.IMGRET_DB_TILE))
    return max(1, min(d_tiles, -(-512 // q_tiles), ops.IMGRET_MAX_SPLITS))


def _vectors(v, device) -> torch.Tensor:
    t = v if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
    if t.dim() != 2:
        raise ValueError(f"expected [n, L] global descriptors, got {tuple(t.shape)}")
    t = t.to(device=device, dtype=torch.float32)
    pad = -int(t.shape[1]) % DIM
    if pad or t.shape[1] == 0:      # zeros add nothing to an inner product
        t = torch.nn.functional.pad(t, (0, pad if t.shape[1] else DIM))
    return t.contiguous()


@torch.no_grad()
def retrieve(query_desc, db_desc, num_matched: int, exclude=None, db_valid=None, splits: Optional[int] = None):
    """query_desc [nq, L], db_desc [nd, L]: any global descriptors (these VLAD vectors, NetVLAD vectors from outside) -> (idx int32
    [nq, num_matched], sim float32 [nq, num_matched]) on the device: per query the database rows of largest inner product,
    similarity descending, then index ascending; -1 / 0 where fewer are allowed.  exclude [nq]: a database index the query may not
    return (-1: none); db_valid [nd]: false bars a row.  ``splits`` only spreads the work; the result does not depend on it."""
    dev = _device(db_desc.device if torch.is_tensor(db_desc) else (query_desc.device if torch.is_tensor(query_desc) else "cuda"))
    q, db = _vectors(query_desc, dev), _vectors(db_desc, dev)
    if q.shape[1] != db.shape[1]:
        raise ValueError(f"retrieve: the descriptors' lengths differ: {q.shape[1]} and {db.shape[1]}")
    nq, nd = int(q.shape[0]), int(db.shape[0])
    if exclude is not None:
        exclude = torch.as_tensor(exclude).to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        if exclude.numel() != nq:
            raise ValueError("retrieve: exclude needs one entry per query")
    if db_valid is not None:
        db_valid = torch.as_tensor(db_valid).to(device=dev).ne(0).to(torch.uint8).contiguous().reshape(-1)
        if db_valid.numel() != nd:
            raise ValueError("retrieve: db_valid needs one entry per database row")
    return ops.imgret_topk(q, db, int(num_matched), exclude, db_valid, default_splits(nq, nd) if splits is None else int(splits))


def pairs_from_retrieval(db_desc, num_matched: int) -> List[Tuple[int, int]]:
    """The image pairs to match, for mapper.reconstruct and formats.match_pairs: every image with its ``num_matched`` most similar
    others (self excluded), a pair listed once, the first occurrence kept in row-major order of the lists
    (formats.find_unique_new_pairs' rule).  One read-back."""
    n = int(db_desc.shape[0])
    idx, _sim = retrieve(db_desc, db_desc, num_matched, exclude=np.arange(n, dtype=np.int32))
    seen, pairs = set(), []
    for i, row in enumerate(idx.cpu().numpy().tolist()):
        for j in row:
            if j >= 0 and (i, j) not in seen and (j, i) not in seen:
                seen.add((i, j))
                pairs.append((i, j))
    return pairs


class RetrievalIndex:
    """The global descriptors of a store's frames (ReferenceStore or DatabaseStore), resident on the store's device."""

    def __init__(self, store, vocab: Vocabulary, image_chunk: int = 1024):
        self.store, self.vocab = store, vocab
        self.descriptors = global_descriptors(vocab, store, image_chunk)

    def query(self, features: dict, num_matched: int) -> List[list]:
        """features: the batched extractor output -> per query the store's frame ids of its ``num_matched`` most similar frames,
        best first: the ``retrieval`` argument of retrieval.localize_by_retrieval.  A query without keypoints gets an empty list."""
        q = global_descriptors(self.vocab, features)
        if q.shape[0] == 0 or self.store.n_frames == 0:
            return [[] for _ in range(int(q.shape[0]))]
        idx, _sim = retrieve(q, self.descriptors, num_matched)
        counts = features["counts"].cpu().numpy().reshape(-1)
        return [[self.store.frame_ids[j] for j in row if j >= 0] if counts[b] > 0 else [] for b, row in enumerate(idx.cpu().numpy().tolist())]
