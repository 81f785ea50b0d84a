"""Config reader and dataset surface of the reference's `data.py`, as far as the encoder hot path
needs it.

`read_config(path) -> Config` parses the reference's experiment .cfg files into the same attribute
bag (reference data.py:15-130: same attribute names, types, defaults, derived values and the same
side effects — experiment folder creation and a copy of the cfg).  It additionally accepts the nine
legacy cfgs the reference's own parser rejects (they carry `dataset_subset_percentage` instead of
the four `*_subset_percentage` keys): the legacy key maps to
`real_dataset_subset_percentage`, the other three default to 1.0.

Datasets: `get_SLU_datasets` / `SLUDataset` / `CollateWavsSLU` read a Fluent-Speech-Commands tree
(CSV splits + wavs) with the reference's split / subset / label-dictionary logic (data.py:132-376;
SURVEY.md §8(f) rank 1), feeding pinned, zero-padded (B, T_max) batches to the encoder; with
`get_ASR_datasets` / `ASRDataset` / `CollateWavsASR` read a LibriSpeech + TextGrid alignment tree
(data.py:393-545).  With `slu_path` / `asr_path = synthetic[:NxBxT]` FSC- / LibriSpeech-shaped SYNTHETIC
datasets with the same duck type are served (`.loader` yielding the same batch tuples;
`training.Trainer` dispatches on `SLUDataset` / `ASRDataset`).
"""
import collections
import configparser
import os
import shutil
from collections import Counter

import numpy as np
import torch

from slu_hip import knobs as _knobs


class Config:
    def __init__(self):
        self.use_sincnet = True


def _ints(s):
    return [int(v) for v in s.split(",")]


def _floats(s):
    return [float(v) for v in s.split(",")]


def _strs(s):
    return [v for v in s.split(",")]


def _flag(s):
    return s == "True"


def _none_or_str(s):
    return None if s == "None" else s


# (section, key, converter) in the reference's reading order; attribute name == key
_REQUIRED = [
    ("phoneme_module", "use_sincnet", _flag), ("phoneme_module", "fs", int),
    ("phoneme_module", "cnn_N_filt", _ints), ("phoneme_module", "cnn_len_filt", _ints),
    ("phoneme_module", "cnn_stride", _ints), ("phoneme_module", "cnn_max_pool_len", _ints),
    ("phoneme_module", "cnn_act", _strs), ("phoneme_module", "cnn_drop", _floats),
    ("phoneme_module", "phone_rnn_num_hidden", _ints), ("phoneme_module", "phone_downsample_len", _ints),
    ("phoneme_module", "phone_downsample_type", _strs), ("phoneme_module", "phone_rnn_drop", _floats),
    ("phoneme_module", "phone_rnn_bidirectional", _flag),
    ("word_module", "word_rnn_num_hidden", _ints), ("word_module", "word_downsample_len", _ints),
    ("word_module", "word_downsample_type", _strs), ("word_module", "word_rnn_drop", _floats),
    ("word_module", "word_rnn_bidirectional", _flag), ("word_module", "vocabulary_size", int),
    ("intent_module", "intent_rnn_num_hidden", _ints), ("intent_module", "intent_downsample_len", _ints),
    ("intent_module", "intent_downsample_type", _strs), ("intent_module", "intent_rnn_drop", _floats),
    ("intent_module", "intent_rnn_bidirectional", _flag),
]
_SEQ2SEQ_KEYS = ["intent_encoder_dim", "num_intent_encoder_layers", "intent_decoder_dim",
                 "num_intent_decoder_layers", "intent_decoder_key_dim", "intent_decoder_value_dim"]
_PRETRAINING = [("asr_path", str), ("pretraining_type", int), ("pretraining_lr", float),
                ("pretraining_batch_size", int), ("pretraining_num_epochs", int),
                ("pretraining_length_mean", float), ("pretraining_length_var", float)]
_TRAINING_HEAD = [("slu_path", str), ("unfreezing_type", int), ("training_lr", float),
                  ("training_batch_size", int), ("training_num_epochs", int)]
_SUBSETS = ["real_dataset_subset_percentage", "synthetic_dataset_subset_percentage",
            "real_speaker_subset_percentage", "synthetic_speaker_subset_percentage"]


def read_config(config_file):
    """Parse an experiment .cfg into a Config (reference data.py:19-130)."""
    parser = configparser.ConfigParser()
    parser.read(config_file)
    config = Config()
    config.seed = int(parser.get("experiment", "seed"))
    config.folder = parser.get("experiment", "folder")

    # side effects of the reference (data.py:29-33): experiment folder + a copy of the cfg
    # (race-free: under torch.distributed every rank calls read_config; only rank 0 copies the cfg)
    for sub in ("", "pretraining", "training"):
        os.makedirs(os.path.join(config.folder, sub), exist_ok=True)
    if int(os.environ.get("RANK", "0")) == 0:
        try:
            shutil.copyfile(config_file, os.path.join(config.folder, "experiment.cfg"))
        except (shutil.SameFileError, OSError):
            pass

    for section, key, conv in _REQUIRED:
        setattr(config, key, conv(parser.get(section, key)))
    try:
        vals = [int(parser.get("intent_module", k)) for k in _SEQ2SEQ_KEYS]
        for k, v in zip(_SEQ2SEQ_KEYS, vals):
            setattr(config, k, v)
    except Exception:
        # partial seq2seq sections leave the earlier keys set, like the reference's sequential reads
        for k in _SEQ2SEQ_KEYS:
            try:
                setattr(config, k, int(parser.get("intent_module", k)))
            except Exception:
                break
        print("no seq2seq hyperparameters")

    for key, conv in _PRETRAINING[:2]:
        setattr(config, key, conv(parser.get("pretraining", key)))
    n_word, n_phone, n_cnn = (len(config.word_rnn_num_hidden), len(config.phone_rnn_num_hidden),
                              len(config.cnn_N_filt))
    start = {0: 1 + n_word + n_phone + n_cnn, 1: 1 + n_word, 2: 1, 3: 1}
    if config.pretraining_type in start:
        config.starting_unfreezing_index = start[config.pretraining_type]
    for key, conv in _PRETRAINING[2:]:
        setattr(config, key, conv(parser.get("pretraining", key)))

    for key, conv in _TRAINING_HEAD:
        setattr(config, key, conv(parser.get("training", key)))
    if parser.has_option("training", _SUBSETS[0]):
        for key in _SUBSETS:
            setattr(config, key, float(parser.get("training", key)))
    elif parser.has_option("training", "dataset_subset_percentage"):
        # legacy cfg (superset of the reference's behaviour, which raises NoOptionError here)
        config.real_dataset_subset_percentage = float(parser.get("training", "dataset_subset_percentage"))
        for key in _SUBSETS[1:]:
            config.__dict__[key] = float(parser.get("training", key)) if parser.has_option("training", key) else 1.0
    else:
        parser.get("training", _SUBSETS[0])          # raises configparser.NoOptionError like the reference
    config.train_wording_path = _none_or_str(parser.get("training", "train_wording_path"))
    config.test_wording_path = _none_or_str(parser.get("training", "test_wording_path"))
    config.augment = _flag(parser.get("training", "augment", fallback="False"))
    config.seq2seq = _flag(parser.get("training", "seq2seq", fallback="False"))
    try:
        config.dataset_upsample_factor = int(parser.get("training", "dataset_upsample_factor"))
    except Exception:
        config.dataset_upsample_factor = 1

    # total time decimation of the phoneme / word modules (reference data.py:121-128)
    config.phone_downsample_factor = 1
    for f in config.cnn_stride + config.cnn_max_pool_len + config.phone_downsample_len:
        config.phone_downsample_factor *= f
    config.word_downsample_factor = config.phone_downsample_factor
    for f in config.word_downsample_len:
        config.word_downsample_factor *= f
    return config


# ------------------------------------------------------------------------------------------------
# synthetic datasets (shape-compatible stand-ins for the reference's wav/CSV loaders)
# ------------------------------------------------------------------------------------------------
FSC_VALUES_PER_SLOT = [6, 14, 4]       # Fluent Speech Commands: action / object / location


def synthetic_Sy_intent(values_per_slot=FSC_VALUES_PER_SLOT):
    names = ["action", "object", "location"]
    return {names[s]: {"%s_%d" % (names[s], v): v for v in range(n)} for s, n in enumerate(values_per_slot)}


class _SyntheticLoader:
    """Iterable of pre-generated batches (one pass per __iter__, like a DataLoader)."""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def pcm16_batches():
    """SLU_PCM16_BATCHES=1: loaders hand PCM16 audio over as int16 batches (B, T) — half the bytes on PCIe; the model's
    first stage computes on sample / 32768 (slu_hip.ops.PCM16_SCALE), which is exactly the float32 value the default
    loaders (and the reference's, data.py:273-293) produce, so losses and parameters are bit-identical.  Off by default:
    code that consumes `dataset.loader` directly keeps seeing the reference's float32 waveforms."""
    return _knobs.get("SLU_PCM16_BATCHES")


def resample_enabled():
    """SLU_RESAMPLE: "0" (default) — a wav file's sample rate is ignored: every file is taken to be sampled at the model's
    config.fs, as in the reference; "1" — SLU datasets keep each file's rate, CollateWavsSLU hands the batch over as a
    SourceWaves and the training loops convert it to config.fs on the device (slu_hip.ops.wave_resample) in front of
    everything else; the ASR pre-training datasets refuse a file at another rate."""
    return _knobs.added("SLU_RESAMPLE")


RatedWave = collections.namedtuple("RatedWave", "x rate")    # an SLUDataset item's waveform under SLU_RESAMPLE=1


class SourceWaves:
    """The first element of an SLU batch under SLU_RESAMPLE=1: the waveforms as the files hold them.  x (B, T_src) host
    tensor (float32, or int16 under SLU_PCM16_BATCHES=1), zero-padded at the end in SOURCE samples; lengths (B) int32
    host tensor, the rows' source sample counts; rates: B ints; target: the rate they are to be converted to; out_T: the
    width of the converted batch (the largest output length, rounded up to SLU_PAD_TO_MULTIPLE); out_lengths: the B
    output lengths (ops.resample_out_lengths).  Everything downstream of the conversion needs is known on the host."""

    def __init__(self, x, lengths, rates, target, out_T, out_lengths):
        self.x, self.lengths, self.rates, self.target = x, lengths, [int(r) for r in rates], int(target)
        self.out_T, self.out_lengths = int(out_T), [int(n) for n in out_lengths]

    def __len__(self):
        return self.x.shape[0]

    def pin_memory(self):
        """What the DataLoader's pinning calls on a batch element it does not know."""
        return SourceWaves(self.x.pin_memory(), self.lengths.pin_memory(), self.rates, self.target, self.out_T,
                           self.out_lengths)


def _require_rate(path, fs, config_fs, who):
    if int(fs) != int(config_fs):
        raise ValueError("resample: %s: %s is sampled at %d Hz, the model at %d Hz; ASR pre-training builds its label "
                         "tracks from the file's own rate and is not converted (SLU_RESAMPLE=1 covers the SLU datasets)"
                         % (who, path, int(fs), int(config_fs)))


def read_wav(path, keep_pcm16=False):
    """First channel of a wav file as float32 in [-1, 1) and its sample rate — the array
    `SoxEffectsChain.sox_build_flow_effects()` hands the reference (data.py:273-293; augmentation is
    hard-wired off there, so the chain is a plain decode): PCM16 / 32768, PCM32 / 2^31, unsigned 8-bit
    (v - 128) / 128, float wavs as stored.  keep_pcm16: PCM16 files come back as the int16 samples themselves."""
    from scipy.io import wavfile
    fs, a = wavfile.read(path)
    if a.ndim > 1:
        a = a[:, 0]
    if a.dtype == np.int16 and keep_pcm16:
        return np.ascontiguousarray(a), fs
    if a.dtype == np.int16:
        x = a.astype(np.float32) / 32768.0
    elif a.dtype == np.int32:
        x = (a.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif a.dtype == np.uint8:
        x = (a.astype(np.float32) - 128.0) / 128.0
    else:
        x = a.astype(np.float32)
    return x, fs


def _pad_waveforms(waves, T):
    """list of 1-D waveforms -> (B, T) zero-padded at the end: int16 when every item is PCM16 samples (pcm16_batches),
    else float32 (int16 items are converted as read_wav would have)."""
    as_np = [np.asarray(w) for w in waves]
    if all(a.dtype == np.int16 for a in as_np):
        x = torch.zeros(len(as_np), T, dtype=torch.int16)
        for i, a in enumerate(as_np):
            x[i, :len(a)] = torch.from_numpy(a)
        return x
    x = torch.zeros(len(as_np), T, dtype=torch.float32)
    for i, a in enumerate(as_np):
        x[i, :len(a)] = torch.from_numpy(a.astype(np.float32) / 32768.0) if a.dtype == np.int16 else torch.as_tensor(a, dtype=torch.float32)
    return x


def one_hot(letters, S):
    """letters (B, U) int64 label indices -> (B, U, S) float32 one-hot rows (reference data.py:331-342)."""
    out = torch.zeros(letters.shape[0], letters.shape[1], S)
    out.scatter_(2, letters.long().unsqueeze(2), 1.0)
    return out


def mask_padding_enabled():
    """SLU_MASK_PADDING: "0" (default) — batches are (x, y); "1" — CollateWavsSLU adds the per-utterance sample counts."""
    return _knobs.get("SLU_MASK_PADDING")


def mask_asr_enabled():
    """SLU_MASK_ASR: "0" (default) — ASR batches are (x, y_phoneme, y_word), also under SLU_MASK_PADDING=1; "1" —
    CollateWavsASR adds the snippets' own sample counts.  Needs SLU_MASK_PADDING=1."""
    on = _knobs.get("SLU_MASK_ASR")
    if on and not mask_padding_enabled():
        raise ValueError("SLU_MASK_ASR=1 needs SLU_MASK_PADDING=1: the lengths come from the collate function")
    return on


def asr_ctc_enabled():
    """SLU_ASR_CTC: "0" (default) — ASR batches carry one label per frame (forced alignments); "1" — they carry label
    SEQUENCES and PretrainedModel trains its heads by CTC (models.asr_ctc_enabled).  Needs SLU_MASK_PADDING=1,
    SLU_MASK_ASR=1 and SLU_MASK_TRAIN=1: CTC needs every utterance's length, in training and in evaluation."""
    on = _knobs.get("SLU_ASR_CTC")
    if on:
        for name in ("SLU_MASK_PADDING", "SLU_MASK_ASR", "SLU_MASK_TRAIN"):
            if not _knobs.get(name):
                raise ValueError("SLU_ASR_CTC=1 needs %s=1: CTC needs the utterances' lengths in training and in evaluation"
                                 % name)
    return on


def ctc_max_seconds():
    """SLU_CTC_MAX_SECONDS (default 20): TranscriptASRDataset skips utterances longer than this."""
    v = _knobs.get("SLU_CTC_MAX_SECONDS")
    try:
        sec = float(v)
    except ValueError:
        sec = -1.0
    if not sec > 0:
        raise ValueError("SLU_CTC_MAX_SECONDS=%r: expected a positive number of seconds" % v)
    return sec


def ctc_collapse(track):
    """A frame-label track -> its label sequence: runs of equal consecutive entries are merged first, -1 (no label)
    counting as an entry, then the -1 are dropped.  A,A,-1,A,B,B -> A,A,B: the track is itself a CTC path of the
    sequence it gives (-1 in the blank's role), so a forced alignment is always feasible for its own frames."""
    out, prev = [], None
    for v in track:
        v = int(v)
        if v != prev and v != -1:
            out.append(v)
        prev = v
    return out


def _pad_sequences(seqs):
    y = torch.full((len(seqs), max([len(s) for s in seqs] + [1])), -1, dtype=torch.int64)
    for i, s in enumerate(seqs):
        if len(s):
            y[i, :len(s)] = torch.as_tensor(np.asarray(s, dtype=np.int64))
    return y


class CollateWavsSLU:
    """list of (waveform, [action, object, location]) -> (x (B, T_max) float32 zero-padded at the end,
    y_intent (B, 3) int64), as reference data.py:344-376.  seq2seq: the labels are <sos> ... <eos> index
    sequences, padded with <eos> to the longest of the batch and returned one-hot, (B, U_max, num_labels) float32
    (data.py:363-376).  The batch is assembled directly in ONE buffer instead of per-row pad + stack; the DataLoader
    pins it (pin_memory=True, in the parent process — never in a forked worker) so that the H2D copy of the
    look-ahead slots is asynchronous."""

    def __init__(self, Sy_intent, seq2seq, pad_multiple=None, mask_padding=None, resample_to=None):
        # SLU_RESAMPLE=1 (SLUDataset passes config.fs): the items' waveforms are RatedWave(x, rate); x of the batch is a
        # SourceWaves padded in SOURCE samples, the lengths (SLU_MASK_PADDING=1) are the CONVERTED ones and
        # SLU_PAD_TO_MULTIPLE rounds the converted width.  None: the batch documented above, whatever the files' rates.
        self.resample_to = None if resample_to is None else int(resample_to)
        self.Sy_intent = Sy_intent
        self.num_labels = len(self.Sy_intent)
        self.seq2seq = seq2seq
        if self.seq2seq:
            self.EOS = self.Sy_intent.index("<eos>")
        # Opt-in (SLU_PAD_TO_MULTIPLE=n samples): round T_max up to a multiple of n so that ragged real
        # data falls into a few batch shapes (the look-ahead super-batches and hipGraphs are per shape).
        # Off by default: the extra trailing zeros are seen by the recurrences, i.e. it is not the
        # reference's batch any more.
        self.pad_multiple = _knobs.get("SLU_PAD_TO_MULTIPLE") if pad_multiple is None else pad_multiple
        # Opt-in (SLU_MASK_PADDING=1): also return the utterances' own sample counts, (x, y, lengths int32 (B)) — taken
        # before the rounding above — so that evaluation can run padding-invariant (Model.eval_group(lengths=...):
        # every utterance's logits are those of the utterance alone, whatever it was batched with).  The training loops
        # drop them (training.Trainer).  Off: the batch is the reference's 2-tuple.
        self.mask_padding = mask_padding_enabled() if mask_padding is None else bool(mask_padding)

    def _source_waves(self, batch):
        from slu_hip import resample as _resample
        waves = [w.x for w, _ in batch]
        rates = [int(w.rate) for w, _ in batch]
        lengths = [len(x) for x in waves]
        n_out = _resample.out_lengths(lengths, rates, self.resample_to)
        T_out = max(n_out)
        if self.pad_multiple > 1:
            T_out = -(-T_out // self.pad_multiple) * self.pad_multiple
        x = SourceWaves(_pad_waveforms(waves, max(lengths)), torch.tensor(lengths, dtype=torch.int32), rates,
                        self.resample_to, T_out, n_out)
        if self.mask_padding:
            x, y = self._labels(batch, x)
            return x, y, torch.tensor(n_out, dtype=torch.int32)
        return self._labels(batch, x)

    def __call__(self, batch):
        if self.resample_to is not None:
            return self._source_waves(batch)
        T = max(len(x) for x, _ in batch)
        if self.pad_multiple > 1:
            T = -(-T // self.pad_multiple) * self.pad_multiple
        x = _pad_waveforms([xi for xi, _ in batch], T)
        if self.mask_padding:
            x, y = self._labels(batch, x)
            return x, y, torch.tensor([len(xi) for xi, _ in batch], dtype=torch.int32)
        return self._labels(batch, x)

    def _labels(self, batch, x):
        if self.seq2seq:
            U = max(len(yi) for _, yi in batch)
            idx = torch.full((len(batch), U), self.EOS, dtype=torch.int64)
            for i, (_, yi) in enumerate(batch):
                idx[i, :len(yi)] = torch.as_tensor(list(yi), dtype=torch.int64)
            return x, one_hot(idx, self.num_labels)
        y = torch.tensor([list(yi) for _, yi in batch], dtype=torch.int64)
        return x, y


def _world():
    """(rank, world size) of the data-parallel job (one process per GPU), (0, 1) outside one."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _loader_workers():
    """The reference starts one DataLoader worker per core (data.py:261); on a 256-thread MI355X host
    that is all start-up cost, so the default is capped (SLU_DATA_WORKERS overrides, 0 = in-process)."""
    n = _knobs.get("SLU_DATA_WORKERS")
    return min(16, os.cpu_count() or 1) if n is None else n


class ForkSafeDataLoader(torch.utils.data.DataLoader):
    """DataLoader whose worker processes are forked from a process that holds GPU objects (hipGraphs, CU-masked streams,
    events, IPC windows).  A forked child must never FINALISE such objects — their destructors call into a HIP runtime
    that does not exist in the child — yet CPython may run a garbage collection right inside the child's fork bootstrap
    (`threading._after_fork`), and any unreachable cycle that holds one of them is then destroyed there: seen once as
    "Fatal Python error: Segmentation fault ... Garbage-collecting" in a worker of the ASR loader.  So: collect in the
    PARENT (where the runtime is alive) right before the workers start, and freeze what exists (`gc.freeze`: the children
    inherit a permanent generation their collections never visit); the parent unfreezes afterwards."""

    def __iter__(self):
        if self.num_workers <= 0:
            return super().__iter__()
        import gc
        gc.collect()
        gc.freeze()
        try:
            return super().__iter__()            # the workers are forked here
        finally:
            gc.unfreeze()


def wav_num_samples(path):
    """Number of frames of a wav file from its header (falls back to decoding for non-PCM files)."""
    import wave
    try:
        with wave.open(path, "rb") as w:
            return w.getnframes()
    except (wave.Error, EOFError):
        return len(read_wav(path)[0])


class LengthBucketBatchSampler(torch.utils.data.Sampler):
    """Opt-in batch sampler for ragged real data (SLU_BUCKET_BATCHES=1 together with
    SLU_PAD_TO_MULTIPLE=n): utterances are bucketed by ceil(length / n), batches are drawn inside a bucket
    (shuffled every epoch) and the batches of one bucket are emitted consecutively, buckets in random
    order.  With the collate function padding to the same multiple, every batch of a bucket has the SAME
    shape and equal shapes are adjacent — which is what lets the look-ahead pipeline form super-batches
    and replay its hipGraphs on real data (it groups consecutive equally-shaped batches).  The price is
    less length mixing inside an epoch than the reference's plain shuffle; off by default.
    Under data parallelism every rank draws the same batch list (seed + epoch) and keeps every
    world-th batch, wrapping around so that all ranks run the same number of steps."""

    def __init__(self, lengths, batch_size, multiple, shuffle=True, generator=None, rank=0, world=1, seed=0):
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.generator = generator
        self.rank, self.world, self.seed, self.epoch = rank, world, seed, 0
        buckets = {}
        for i, n in enumerate(lengths):
            buckets.setdefault(-(-int(n) // int(multiple)), []).append(i)
        self.buckets = [buckets[k] for k in sorted(buckets)]

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _total(self):
        return sum(-(-len(b) // self.batch_size) for b in self.buckets)

    def __len__(self):
        return -(-self._total() // self.world)

    def _batches(self, g):
        order = torch.randperm(len(self.buckets), generator=g).tolist() if self.shuffle else range(len(self.buckets))
        for k in order:
            idx = self.buckets[k]
            if self.shuffle:
                idx = [idx[j] for j in torch.randperm(len(idx), generator=g).tolist()]
            for s0 in range(0, len(idx), self.batch_size):
                yield idx[s0:s0 + self.batch_size]

    def __iter__(self):
        if self.world == 1:
            yield from self._batches(self.generator)
            return
        g = torch.Generator().manual_seed(self.seed + self.epoch)       # the same list on every rank
        batches = list(self._batches(g))
        for k in range(len(self)):
            yield batches[(self.rank + k * self.world) % len(batches)]


class SLUDataset(torch.utils.data.Dataset):
    """Fluent-Speech-Commands-style dataset (reference data.py:246-329): rows of `df` (columns path,
    action, object, location), wavs under `base_path`; item = (float32 waveform, [3 label indices]);
    `len` = rows x upsample_factor; `.loader` = shuffling DataLoader with CollateWavsSLU."""

    def __init__(self, df, base_path, Sy_intent, config, upsample_factor=1, shard=False):
        self.df = df
        self.base_path = base_path
        self.Sy_intent = Sy_intent
        self.upsample_factor = upsample_factor
        self.augment = False
        self.SNRs = [0, 5, 10, 15, 20]
        self.seq2seq = config.seq2seq
        # label lookup and paths as plain lists: no per-item DataFrame indexing in the workers
        self._paths = [os.path.join(base_path, p) for p in df["path"].tolist()]
        if self.seq2seq:
            self._values = [str(v) for v in df["semantics"].tolist()]
            self._index = {c: i for i, c in enumerate(self.Sy_intent)}       # label -> index (list.index per char otherwise)
        else:
            self._values = list(zip(df["action"].tolist(), df["object"].tolist(), df["location"].tolist()))
        # SLU_RESAMPLE=1: the items keep their files' rates; read once, here, so that the workers and the collate agree
        self.resample_to = int(config.fs) if resample_enabled() else None
        collate = CollateWavsSLU(self.Sy_intent, self.seq2seq, resample_to=self.resample_to)
        pin = torch.cuda.is_available()
        # Data parallelism (`shard`: the training split only): every rank draws a disjoint 1/world of the
        # epoch (DistributedSampler pads by repetition so that all ranks run the same number of steps);
        # validation / test stay whole on every rank, so their metrics are the single-process ones.
        rank, world = _world() if shard else (0, 1)
        seed = getattr(config, "seed", 0)
        if _knobs.get("SLU_BUCKET_BATCHES") and collate.pad_multiple > 1:
            if self.resample_to is None:
                lengths = [wav_num_samples(p) for p in self._paths] * self.upsample_factor
            else:                                # bucket by what the model will see: the converted lengths
                from slu_hip import resample as _resample
                frames_rates = [_wav_frames_rate(p) for p in self._paths]
                lengths = _resample.out_lengths([max(1, n) for n, _ in frames_rates], [fs for _, fs in frames_rates],
                                                self.resample_to) * self.upsample_factor
            self.loader = ForkSafeDataLoader(
                self, num_workers=_loader_workers(), collate_fn=collate, pin_memory=pin,
                batch_sampler=LengthBucketBatchSampler(lengths, config.training_batch_size, collate.pad_multiple,
                                                       rank=rank, world=world, seed=seed))
        elif world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(self, num_replicas=world, rank=rank,
                                                                      shuffle=True, seed=seed)
            self.loader = ForkSafeDataLoader(
                self, batch_size=config.training_batch_size, num_workers=_loader_workers(), sampler=sampler,
                collate_fn=collate, pin_memory=pin)
        else:
            self.loader = ForkSafeDataLoader(
                self, batch_size=config.training_batch_size, num_workers=_loader_workers(), shuffle=True,
                collate_fn=collate, pin_memory=pin)

    def __len__(self):
        return len(self._paths) * self.upsample_factor

    def __getitem__(self, idx):
        idx = idx % len(self._paths)
        x, _fs = read_wav(self._paths[idx], keep_pcm16=pcm16_batches())
        if getattr(self, "resample_to", None) is not None:
            x = RatedWave(x, int(_fs))
        if self.seq2seq:                         # <sos> + the characters of the semantics string + <eos> (data.py:322-326)
            y_intent = [self._index["<sos>"]] + [self._index[c] for c in self._values[idx]] + [self._index["<eos>"]]
            return x, y_intent
        # a slot value that never occurs in the training split raises KeyError here, as in the reference
        y_intent = [self.Sy_intent[slot][v] for slot, v in zip(("action", "object", "location"), self._values[idx])]
        return x, y_intent


class SyntheticSLUDataset(SLUDataset):
    """Synthetic SLU dataset: `.loader` yields (x (B,T) float32, y_intent (B,3) int64) like
    CollateWavsSLU (reference data.py:344-376): zero-mean 0.1-RMS noise waveforms, uniform labels."""

    def __init__(self, num_batches, batch_size, num_samples, values_per_slot=FSC_VALUES_PER_SLOT,
                 seed=1234, Sy_intent=None, pin=False):
        g = torch.Generator().manual_seed(seed)
        self.Sy_intent = Sy_intent or synthetic_Sy_intent(values_per_slot)
        self.seq2seq = False
        batches = []
        for _ in range(num_batches):
            x = 0.1 * torch.randn(batch_size, num_samples, generator=g)
            y = torch.stack([torch.randint(0, n, (batch_size,), generator=g) for n in values_per_slot], dim=1)
            if pin and torch.cuda.is_available():
                x, y = x.pin_memory(), y.pin_memory()
            batches.append((x, y))
        self.batches = batches
        self.loader = _SyntheticLoader(batches)

    def __len__(self):
        return sum(len(b[0]) for b in self.batches)

    def __getitem__(self, idx):
        bs = len(self.batches[0][0])
        x, y = self.batches[idx // bs]
        return x[idx % bs], y[idx % bs]


SYNTHETIC_SEQ2SEQ_LABELS = ["<sos>"] + list("abcdefghijklmnopqrstuvwxyz {}:'|,_") + ["<eos>"]


class SyntheticSeq2SeqDataset(SLUDataset):
    """Synthetic seq2seq SLU dataset: `.loader` yields (x (B,T) float32, y (B,U,num_labels) one-hot float32) like
    CollateWavsSLU's seq2seq branch (reference data.py:363-376): noise waveforms, random label strings of 3..U-2
    characters between <sos> and <eos>, padded with <eos>."""

    def __init__(self, num_batches, batch_size, num_samples, max_len=24, seed=1234, Sy_intent=None):
        g = torch.Generator().manual_seed(seed)
        self.Sy_intent = Sy_intent or list(SYNTHETIC_SEQ2SEQ_LABELS)
        self.seq2seq = True
        V = len(self.Sy_intent)
        sos, eos = self.Sy_intent.index("<sos>"), self.Sy_intent.index("<eos>")
        inner = [i for i in range(V) if i not in (sos, eos)]
        batches = []
        for _ in range(num_batches):
            x = 0.1 * torch.randn(batch_size, num_samples, generator=g)
            idx = torch.full((batch_size, max_len), eos, dtype=torch.int64)
            idx[:, 0] = sos
            lens = torch.randint(3, max_len - 1, (batch_size,), generator=g)
            pick = torch.randint(0, len(inner), (batch_size, max_len), generator=g)
            for b in range(batch_size):
                n = int(lens[b])
                idx[b, 1:1 + n] = torch.tensor([inner[int(k)] for k in pick[b, :n]])
            batches.append((x, one_hot(idx, V)))
        self.batches = batches
        self.loader = _SyntheticLoader(batches)

    def __len__(self):
        return sum(len(b[0]) for b in self.batches)

    def __getitem__(self, idx):
        bs = len(self.batches[0][0])
        x, y = self.batches[idx // bs]
        return x[idx % bs], y[idx % bs]


def intent_lexicon(dataset):
    """The sorted unique semantics strings of a seq2seq SLU dataset: the closed set its targets come from (31 on Fluent
    Speech Commands), what Model.set_lexicon takes.  A synthetic dataset's strings are read off its one-hot targets."""
    if not getattr(dataset, "seq2seq", False):
        raise ValueError("intent_lexicon: the dataset has no seq2seq targets")
    if hasattr(dataset, "_values"):
        return sorted(set(dataset._values))
    S = dataset.Sy_intent
    sos, eos = S.index("<sos>"), S.index("<eos>")
    strings = set()
    for _, y in dataset.batches:
        for row in y.max(dim=2)[1].tolist():
            row = row[1:] if row and row[0] == sos else row
            strings.add("".join(S[c] for c in (row[:row.index(eos)] if eos in row else row)))
    return sorted(strings)


def intent_set(dataset):
    """The sorted unique slot-index tuples of a fixed-slot SLU dataset: the closed set its targets come from (31 of the
    6 x 14 x 4 combinations on Fluent Speech Commands), what Model.set_intent_set takes.  A real dataset's tuples are its
    dataframe's (action, object, location) rows through Sy_intent (a value Sy_intent does not know raises KeyError, as
    __getitem__ does); a synthetic dataset's are read off its targets."""
    if getattr(dataset, "seq2seq", False):
        raise ValueError("intent_set: the dataset has seq2seq targets, not slots (see intent_lexicon)")
    if hasattr(dataset, "_values"):
        S = dataset.Sy_intent
        return sorted({tuple(int(S[slot][v]) for slot, v in zip(("action", "object", "location"), row))
                       for row in set(dataset._values)})
    return sorted({tuple(int(v) for v in row) for _, y in dataset.batches for row in y.tolist()})


def read_textgrid(path):
    """Interval tiers of a Praat TextGrid (the long "ooTextFile" format the Montreal Forced Aligner writes
    for LibriSpeech): {tier name: [(minTime, maxTime, mark), ...]}; the first tier of a name wins, like
    `textgrid.TextGrid().getList(name)[0]` in the reference (data.py:478-497).  Point tiers are skipped."""
    import re
    tiers, cur, t0, t1, is_interval = {}, None, None, None, False
    num = r"([-+0-9.eE]+)"
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        for raw in f:
            ln = raw.strip()
            m = re.match(r'class = "(\w+)"', ln)
            if m:
                is_interval = m.group(1) == "IntervalTier"
                cur = None
                continue
            m = re.match(r'name = "(.*)"$', ln)
            if m and is_interval:
                name = m.group(1)
                cur = tiers.setdefault(name, []) if name not in tiers else []    # later duplicates are ignored
                continue
            if cur is None:
                continue
            m = re.match(r"xmin = " + num, ln)
            if m:
                t0 = float(m.group(1))
                continue
            m = re.match(r"xmax = " + num, ln)
            if m:
                t1 = float(m.group(1))
                continue
            m = re.match(r'text = "(.*)"$', ln)
            if m:
                cur.append((t0, t1, m.group(1).replace('""', '"')))
    return tiers


def _strip_stress(mark):
    return mark.rstrip("0123456789")


# ---- CTC forced alignment -> frame labels and TextGrids ("CTC forced alignment") ----------------------
def _label_end(pos):
    """The frame behind the last frame that sits on a label (0: the path is all blanks)."""
    return max((t + 1 for t, p in enumerate(pos) if p >= 0), default=0)


def frame_labels(starts, labels, n_frames, fill="hold", pos=None):
    """One label per frame from an alignment (PretrainedModel.align_phonemes(..., want_pos=True)): starts[j] the first
    frame of labels[j], pos[t] the target position at frame t or -1 on a blank -> n_frames ints, -1 = no label.
    fill="hold" (the project's own rule: CTC paths are peaky, most frames of a label sit on blanks): labels[j] lasts
    from starts[j] to starts[j + 1]; the last one to the end of its own frames; the frames before the first label and the
    trailing blank run are -1.  fill="none": only the frames on the label itself carry it.
    pos is MANDATORY wherever there is a label, for both rules (the end of the last label's own frames, and which frames
    are blanks, are known from it alone): without it, or with a pos of another length, the call is a ValueError.  Only
    an empty target (all frames -1) needs none."""
    if fill not in ("hold", "none"):
        raise ValueError("frame_labels: fill must be 'hold' or 'none', got %r" % (fill,))
    out = [-1] * int(n_frames)
    if len(labels) == 0:
        return out
    if pos is None or len(pos) != n_frames or len(starts) != len(labels):
        raise ValueError("frame_labels: needs pos (n_frames entries) and one start per label")
    if fill == "none":
        return [int(labels[p]) if p >= 0 else -1 for p in pos]
    bounds = [int(v) for v in starts] + [_label_end(pos)]
    for j, lab in enumerate(labels):
        for t in range(bounds[j], bounds[j + 1]):
            out[t] = int(lab)
    return out


def write_textgrid(path, tiers, xmax):
    """The long "ooTextFile" format read_textgrid parses: tiers = {name: [(t0, t1, mark), ...]} with increasing times
    inside [0, xmax].  ASRDataset._track ignores absolute times and concatenates round((t1 - t0) fs) repeats, so every
    tier is made to tile [0, xmax]: gaps become "" intervals (read back as -1), empty intervals are dropped.  Times are
    written with repr(float), which float() reads back to the bit.  A quote in a mark is doubled (read_textgrid undoes
    it); a tier name with a quote is refused, since the reader takes names as they stand."""
    xmax = float(xmax)
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0.0", "xmax = %r" % xmax, "tiers? <exists>",
           "size = %d" % len(tiers), "item []:"]
    for k, (name, intervals) in enumerate(tiers.items()):
        if '"' in name or "\n" in name:                  # read_textgrid takes a tier's name as it stands, unescaped
            raise ValueError("write_textgrid: tier name %r holds a quote or a line break" % (name,))
        tiled, at = [], 0.0
        for t0, t1, mark in intervals:
            t0, t1 = float(t0), float(t1)
            if t0 < at or t1 < t0 or t1 > xmax:
                raise ValueError("write_textgrid: tier %r: interval (%r, %r) overlaps its predecessor or leaves [0, %r]"
                                 % (name, t0, t1, xmax))
            if t0 > at:
                tiled.append((at, t0, ""))
            if t1 > t0:
                tiled.append((t0, t1, str(mark)))
            at = t1
        if at < xmax:
            tiled.append((at, xmax, ""))
        out += ["    item [%d]:" % (k + 1), '        class = "IntervalTier"', '        name = "%s"' % name,
                "        xmin = 0.0", "        xmax = %r" % xmax, "        intervals: size = %d" % len(tiled)]
        for i, (t0, t1, mark) in enumerate(tiled):
            out += ["        intervals [%d]:" % (i + 1), "            xmin = %r" % t0, "            xmax = %r" % t1,
                    '            text = "%s"' % mark.replace('"', '""')]
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(out) + "\n")


def alignment_tiers(starts, pos, words, lexicon, Sy_phoneme, num_samples, fs, factor):
    """The two tiers of one utterance from its phoneme alignment (align_phonemes(..., want_pos=True): starts, pos) ->
    ({"words": [...], "phones": [...]}, xmax) for write_textgrid.  words: the transcript; the aligned labels are
    TranscriptASRDataset's — the lexicon's phonemes of every word that are in Sy_phoneme, in order.  Frame t covers the
    samples [t factor, (t + 1) factor), cut at num_samples; times are samples / fs.
    phones: frame_labels' "hold" rule, marks = the Sy_phoneme strings.  words: derived from the same alignment — a word
    spans from its first phoneme's start to the next aligned word's start, the last one to the end of its last phoneme's
    hold; a word without aligned phonemes gets no interval; marks = the transcript's words, so the reader maps
    out-of-vocabulary words to -1 as it does for forced alignments made elsewhere."""
    index = {}
    for i, v in enumerate(Sy_phoneme):
        index.setdefault(v, i)
    per_word = [[index[p] for p in lexicon.get(w, ()) if p in index] for w in words]
    labels = [v for ph in per_word for v in ph]
    if len(labels) != len(starts):
        raise ValueError("alignment_tiers: %d starts for %d phonemes of the transcript" % (len(starts), len(labels)))
    ell = int(num_samples)
    at = lambda frame: min(int(frame) * int(factor), ell) / float(fs)
    bounds = [int(v) for v in starts] + [_label_end(pos)]
    phones = [(at(bounds[j]), at(bounds[j + 1]), Sy_phoneme[lab]) for j, lab in enumerate(labels)]
    first, j = [], 0
    for w, ph in zip(words, per_word):
        if ph:
            first.append((w, bounds[j]))
        j += len(ph)
    word_tier = [(at(f0), at(first[k + 1][1] if k + 1 < len(first) else bounds[-1]), w) for k, (w, f0) in enumerate(first)]
    return {"words": word_tier, "phones": phones}, ell / float(fs)


class CollateWavsASR:
    """list of (waveform, phoneme labels, word labels) -> (x (B,T_max) float32 zero-padded, y_phoneme
    (B,U_p) int64, y_word (B,U_w) int64, both padded with the ignore index -1) — reference data.py:511-545.
    Assembled in one buffer per tensor (pinned by the DataLoader).
    Opt-in (SLU_MASK_ASR=1, with SLU_MASK_PADDING=1; or mask_asr=True): also return the snippets' own sample counts, (x,
    y_phoneme, y_word, lengths int32 (B)), so that PretrainedModel.forward(lengths=...) can skip the padded frames.
    pad_multiple (samples; 0, the default and what ASRDataset uses: none) rounds T_max up to a multiple, and the label
    tracks follow by the dataset's own rule, one label per factors = (phone, word downsample factor) samples: with lengths
    a masked step must not depend on how far its batch is padded, and this is how a test pads it further.
    Opt-in (SLU_ASR_CTC=1, or ctc=True): (x, y_phoneme_seq (B, S_p), y_word_seq (B, S_w), lengths) — each label track
    collapsed to its label sequence (ctc_collapse), padded with -1; sequences=True: the items carry label sequences
    already (TranscriptASRDataset), taken as they are."""

    def __init__(self, mask_asr=None, pad_multiple=0, factors=None, ctc=None, sequences=False):
        self.ctc = asr_ctc_enabled() if ctc is None else bool(ctc)
        self.sequences = bool(sequences)
        self.mask_asr = self.ctc or (mask_asr_enabled() if mask_asr is None else bool(mask_asr))
        self.pad_multiple = int(pad_multiple)
        if self.pad_multiple > 1 and factors is None:
            raise ValueError("CollateWavsASR: pad_multiple needs factors = (phone_downsample_factor, word_downsample_factor)")
        self.factors = factors

    def __call__(self, batch):
        n = len(batch)
        T = max(len(b[0]) for b in batch)
        Up = max(len(b[1]) for b in batch)
        Uw = max(len(b[2]) for b in batch)
        if self.pad_multiple > 1:
            T = -(-T // self.pad_multiple) * self.pad_multiple
            Up, Uw = max(Up, -(-T // self.factors[0])), max(Uw, -(-T // self.factors[1]))
        x = _pad_waveforms([b[0] for b in batch], T)
        if self.ctc:
            seq = (lambda t: [int(v) for v in t]) if self.sequences else ctc_collapse
            return (x, _pad_sequences([seq(b[1]) for b in batch]), _pad_sequences([seq(b[2]) for b in batch]),
                    torch.tensor([len(b[0]) for b in batch], dtype=torch.int32))
        yp = torch.full((n, Up), -1, dtype=torch.int64)
        yw = torch.full((n, Uw), -1, dtype=torch.int64)
        for i, (xi, pi, wi) in enumerate(batch):
            yp[i, :len(pi)] = torch.as_tensor(np.asarray(pi, dtype=np.int64))
            yw[i, :len(wi)] = torch.as_tensor(np.asarray(wi, dtype=np.int64))
        if self.mask_asr:
            return x, yp, yw, torch.tensor([len(b[0]) for b in batch], dtype=torch.int32)
        return x, yp, yw


class ASRDataset(torch.utils.data.Dataset):
    """LibriSpeech + forced-alignment dataset of ASR pre-training (reference data.py:453-509): item =
    a random snippet of the utterance (length ~ N(mean, var) seconds, at least 0.5 s; torch's global RNG,
    consumed in the reference's order) with one phoneme label per `phone_downsample_factor` samples and
    one word label per `word_downsample_factor` samples; -1 = no label (silence / out-of-vocabulary).
    Label lookup is a dictionary (first index wins, like list.index) and the per-sample label tracks are
    numpy repeats instead of Python lists."""

    def __init__(self, wav_paths, textgrid_paths, Sy_phoneme, Sy_word, config, shard=False):
        self.wav_paths = wav_paths
        self.textgrid_paths = textgrid_paths
        self.length_mean = config.pretraining_length_mean
        self.length_var = config.pretraining_length_var
        self.Sy_phoneme = Sy_phoneme
        self.Sy_word = Sy_word
        self.phone_downsample_factor = config.phone_downsample_factor
        self.word_downsample_factor = config.word_downsample_factor
        self.require_fs = int(config.fs) if resample_enabled() else None     # SLU_RESAMPLE=1: refuse, do not mistrain
        self._phone_idx, self._word_idx = {}, {}
        for i, v in enumerate(Sy_phoneme):
            self._phone_idx.setdefault(v, i)
        for i, v in enumerate(Sy_word):
            self._word_idx.setdefault(v, i)
        rank, world = _world() if shard else (0, 1)          # training split under data parallelism
        if world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(self, num_replicas=world, rank=rank,
                                                                      shuffle=True, seed=getattr(config, "seed", 0))
            self.loader = ForkSafeDataLoader(
                self, batch_size=config.pretraining_batch_size, num_workers=_loader_workers(), sampler=sampler,
                collate_fn=CollateWavsASR(), pin_memory=torch.cuda.is_available())
        else:
            self.loader = ForkSafeDataLoader(
                self, batch_size=config.pretraining_batch_size, num_workers=_loader_workers(), shuffle=True,
                collate_fn=CollateWavsASR(), pin_memory=torch.cuda.is_available())

    def __len__(self):
        return len(self.wav_paths)

    @staticmethod
    def _track(intervals, index_of, fs):
        idx = np.array([index_of(mark) for _, _, mark in intervals], dtype=np.int64)
        reps = np.array([max(0, round((t1 - t0) * fs)) for t0, t1, _ in intervals], dtype=np.int64)
        return np.repeat(idx, reps)

    def __getitem__(self, idx):
        x32, fs = read_wav(self.wav_paths[idx])
        if getattr(self, "require_fs", None) is not None:
            _require_rate(self.wav_paths[idx], fs, self.require_fs, "ASRDataset")
        x = x32.astype(np.float64)                     # soundfile.read hands the reference float64
        tg = read_textgrid(self.textgrid_paths[idx])
        y_phoneme = self._track(tg["phones"], lambda m: -1 if m == "" else self._phone_idx.get(_strip_stress(m), -1), fs)
        y_word = self._track(tg["words"], lambda m: self._word_idx.get(m, -1), fs)
        random_length = round(fs * max(self.length_mean + self.length_var * torch.randn(1).item(), 0.5))
        if len(x) <= random_length:
            start = 0
        else:
            start = torch.randint(low=0, high=len(x) - random_length, size=(1,)).item()
        end = start + random_length
        return (x[start:end], y_phoneme[start:end:self.phone_downsample_factor].tolist(),
                y_word[start:end:self.word_downsample_factor].tolist())


class SyntheticASRDataset(ASRDataset):
    """Synthetic ASR pre-training dataset: `.loader` yields (x (B,T), y_phoneme (B,ceil(T/640)),
    y_word (B,ceil(T/2560))) like CollateWavsASR (reference data.py:511-545); 10 % of the frame
    labels are the ignore index -1."""

    def __init__(self, num_batches, batch_size, num_samples, config, seed=1234):
        g = torch.Generator().manual_seed(seed)
        Tp = -(-num_samples // config.phone_downsample_factor)
        Tw = -(-num_samples // config.word_downsample_factor)
        batches = []
        for _ in range(num_batches):
            x = 0.1 * torch.randn(batch_size, num_samples, generator=g)
            yp = torch.randint(0, config.num_phonemes, (batch_size, Tp), generator=g)
            yw = torch.randint(0, config.vocabulary_size, (batch_size, Tw), generator=g)
            yp[torch.rand(batch_size, Tp, generator=g) < 0.1] = -1
            yw[torch.rand(batch_size, Tw, generator=g) < 0.1] = -1
            if asr_ctc_enabled():
                # the same draws, served as CollateWavsASR serves an aligned corpus under the knob: ragged sample counts (the
                # waveforms are zero beyond them), the tracks cut to the frames inside them and collapsed
                n = torch.randint(num_samples // 2, num_samples + 1, (batch_size,), generator=g)
                n[0] = num_samples
                x = x * (torch.arange(num_samples).unsqueeze(0) < n.unsqueeze(1))
                cut = lambda y, f: _pad_sequences([ctc_collapse(y[i, :max(1, int(n[i]) // f)].tolist())
                                                   for i in range(batch_size)])
                batches.append((x, cut(yp, config.phone_downsample_factor), cut(yw, config.word_downsample_factor),
                                n.to(torch.int32)))
                continue
            batches.append((x, yp, yw))
        self.batches = batches
        self.loader = _SyntheticLoader(batches)

    def __len__(self):
        return sum(len(b[0]) for b in self.batches)

    def __getitem__(self, idx):
        bs = len(self.batches[0][0])
        b = self.batches[idx // bs]
        return tuple(t[idx % bs] for t in b)


CTC_MAX_LABELS = 255        # 2 S + 1 <= 512 states: what slu_ctc_loss_fwd is instantiated for


def read_lexicon(path):
    """A pronunciation lexicon in CMUdict text format — `WORD  PH PH ...` per line, `;;;` comments, alternative
    pronunciations as WORD(2) (the first one wins) — -> {WORD: [phoneme, ...]} with the stress digits stripped."""
    lex = {}
    with open(path, "r", encoding="latin-1") as f:
        for ln in f:
            parts = ln.split()
            if not parts or ln.startswith(";;;"):
                continue
            word = parts[0].split("(")[0]
            lex.setdefault(word, [_strip_stress(ph) for ph in parts[1:]])
    return lex


def read_transcripts(audio_root, split):
    """LibriSpeech's own transcripts: audio/<split>*/<spk>/<chap>/<spk>-<chap>.trans.txt, lines `<utt-id> WORD WORD ...`
    -> sorted [(wav path, [WORD, ...])] of the utterances whose .wav file exists."""
    import glob
    items = []
    for tr in sorted(glob.glob(os.path.join(audio_root, split + "*", "*", "*", "*.trans.txt"))):
        with open(tr, "r") as f:
            for ln in f:
                parts = ln.split()
                if not parts:
                    continue
                wav = os.path.join(os.path.dirname(tr), parts[0] + ".wav")
                if os.path.isfile(wav):
                    items.append((wav, parts[1:]))
    return sorted(items)


class TranscriptASRDataset(ASRDataset):
    """ASR pre-training without alignments (SLU_ASR_CTC=1): item = a WHOLE utterance (a transcript cannot be cut) with its
    word-index sequence (out-of-vocabulary words dropped) and its phoneme-index sequence through the lexicon (a word
    without an entry contributes no phonemes).  Utterances longer than SLU_CTC_MAX_SECONDS, or with more than
    CTC_MAX_LABELS labels, are skipped, with one printed count.  `.loader` yields CollateWavsASR's CTC batches."""

    def __init__(self, items, Sy_phoneme, Sy_word, lexicon, config, shard=False):
        self._phone_idx, self._word_idx = {}, {}
        for i, v in enumerate(Sy_phoneme):
            self._phone_idx.setdefault(v, i)
        for i, v in enumerate(Sy_word):
            self._word_idx.setdefault(v, i)
        self.Sy_phoneme, self.Sy_word = Sy_phoneme, Sy_word
        limit, kept, skipped = ctc_max_seconds(), [], 0
        require_fs = int(config.fs) if resample_enabled() else None          # SLU_RESAMPLE=1: refuse, do not mistrain
        for wav, words in items:
            n, fs = _wav_frames_rate(wav)
            if require_fs is not None:
                _require_rate(wav, fs, require_fs, "TranscriptASRDataset")
            wd = [self._word_idx[w] for w in words if w in self._word_idx]
            ph = [self._phone_idx[p] for w in words for p in lexicon.get(w, ()) if p in self._phone_idx]
            if n > limit * fs or n < 1 or max(len(wd), len(ph)) > CTC_MAX_LABELS:
                skipped += 1
                continue
            kept.append((wav, ph, wd))
        if skipped:
            print("TranscriptASRDataset: skipped %d of %d utterances (longer than %g s or more than %d labels)"
                  % (skipped, len(items), limit, CTC_MAX_LABELS))
        self.items = kept
        self.wav_paths = [k[0] for k in kept]
        rank, world = _world() if shard else (0, 1)
        collate = CollateWavsASR(ctc=True, sequences=True)
        kw = dict(batch_size=config.pretraining_batch_size, num_workers=_loader_workers(), collate_fn=collate,
                  pin_memory=torch.cuda.is_available())
        if world > 1:
            kw["sampler"] = torch.utils.data.distributed.DistributedSampler(self, num_replicas=world, rank=rank, shuffle=True,
                                                                            seed=getattr(config, "seed", 0))
        else:
            kw["shuffle"] = shard
        self.loader = ForkSafeDataLoader(self, **kw)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        wav, ph, wd = self.items[idx]
        x32, _ = read_wav(wav)
        return x32.astype(np.float64), ph, wd


def _wav_frames_rate(path):
    from scipy.io import wavfile
    fs, a = wavfile.read(path, mmap=True)
    return int(a.shape[0]), int(fs)


def _transcript_datasets(config):
    """get_ASR_datasets without alignments: the vocabularies from <folder>/pretraining/{words,phonemes}.txt, or built from
    the dev split's transcripts (the vocabulary_size most common words; the lexicon's phonemes in first-seen order)."""
    audio = os.path.join(config.asr_path, "audio")
    splits = {k: read_transcripts(audio, k) for k in ("train", "dev", "test")}
    lex_file = os.path.join(config.folder, "pretraining", "lexicon.txt")
    if not os.path.isfile(lex_file):
        raise ValueError("SLU_ASR_CTC=1 without alignments needs a pronunciation lexicon (CMUdict text format) at %s" % lex_file)
    lexicon = read_lexicon(lex_file)
    ph_file = os.path.join(config.folder, "pretraining", "phonemes.txt")
    wd_file = os.path.join(config.folder, "pretraining", "words.txt")
    rank, world = _world()
    if world > 1:
        import torch.distributed as dist
        if rank != 0:
            dist.barrier()
    if os.path.isfile(wd_file):
        with open(wd_file, "r") as f:
            Sy_word = [ln.rstrip("\n") for ln in f.readlines()]
    else:
        counter = Counter(w for _, words in splits["dev"] for w in words)
        Sy_word = [w for w, _ in counter.most_common(config.vocabulary_size)]
        with open(wd_file, "w") as f:
            f.writelines(w + "\n" for w in Sy_word)
    if os.path.isfile(ph_file):
        with open(ph_file, "r") as f:
            Sy_phoneme = [ln.rstrip("\n") for ln in f.readlines() if ln.rstrip("\n") != ""]
    else:
        Sy_phoneme = list(dict.fromkeys(p for _, words in splits["dev"] for w in words for p in lexicon.get(w, ())))
        with open(ph_file, "w") as f:
            f.writelines(p + "\n" for p in Sy_phoneme)
    if world > 1 and rank == 0:
        dist.barrier()
    config.num_phonemes = len(Sy_phoneme)
    mk = lambda k, shard=False: TranscriptASRDataset(splits[k], Sy_phoneme, Sy_word, lexicon, config, shard=shard)
    return mk("train", True), mk("dev"), mk("test")


def _synthetic_spec(path):
    """"synthetic" or "synthetic:<batches>x<batch>x<samples>" -> (batches, batch, samples) or None."""
    if not path.startswith("synthetic"):
        return None
    spec = path.split(":", 1)[1] if ":" in path else ""
    if not spec:
        return 8, None, 48000
    nb, bs, ns = (int(v) for v in spec.split("x"))
    return nb, bs, ns


def _select_rows(df, count):
    """`df.loc[np.random.choice(len(df), count, replace=False)]` of the reference (data.py:174,178):
    label-based, which equals positional selection on a freshly read csv.  After a speaker subset of the
    same csv the index has gaps and the reference raises KeyError; here the rows are then taken by
    position (documented superset)."""
    pick = np.random.choice(len(df), count, replace=False)
    if df.index.is_unique and set(pick).issubset(set(df.index)):
        return df.loc[pick]
    return df.iloc[pick]


def _speaker_subset(df, fraction):
    speakers = np.array(list(Counter(df.speakerId)))
    np.random.shuffle(speakers)
    selected = speakers[:round(fraction * len(speakers))]
    return df[df["speakerId"].isin(selected)]


def _read_phoneme_count(config):
    phonemes = os.path.join(config.folder, "pretraining", "phonemes.txt")
    if os.path.isfile(phonemes):
        with open(phonemes) as f:
            return len([ln for ln in f.read().split("\n") if ln != ""])
    print("No phoneme file found.")
    return None


def get_SLU_datasets(config):
    """(train, valid, test) SLU datasets; also sets config.values_per_slot / Sy_intent /
    num_phonemes (reference data.py:132-240).  `slu_path` is a Fluent-Speech-Commands tree
    (data/{synthetic,train,valid,test}_data.csv + wavs) or `synthetic[:NxBxT]`.  The numpy global RNG is
    consumed in the reference's order (speaker shuffles, then row choices), so a seeded run selects the
    same subsets."""
    import pandas as pd
    spec = _synthetic_spec(config.slu_path)
    if spec is not None:
        nb, bs, ns = spec
        bs = bs or config.training_batch_size
        config.values_per_slot = list(FSC_VALUES_PER_SLOT)
        config.Sy_intent = synthetic_Sy_intent(config.values_per_slot)
        n_ph = _read_phoneme_count(config)
        config.num_phonemes = 42 if n_ph is None else n_ph
        mk = lambda n, seed: SyntheticSLUDataset(n, bs, ns, config.values_per_slot, seed=seed,
                                                 Sy_intent=config.Sy_intent)
        rank = _world()[0]                                  # every rank its own training batches
        if config.seq2seq:
            config.Sy_intent = list(SYNTHETIC_SEQ2SEQ_LABELS)
            mk = lambda n, seed: SyntheticSeq2SeqDataset(n, bs, ns, seed=seed, Sy_intent=config.Sy_intent)
        return (mk(nb, config.seed + 1000003 * rank), mk(max(1, nb // 4), config.seed + 1),
                mk(max(1, nb // 4), config.seed + 2))
    base_path = config.slu_path
    sfx = "_seq2seq" if config.seq2seq else ""          # reference data.py:139-146, 182-187
    csv = lambda name: pd.read_csv(os.path.join(base_path, "data", name.replace(".csv", sfx + ".csv")))
    synthetic_train_df = csv("synthetic_data.csv")
    real_train_df = csv("train_data.csv")
    have_spk = "speakerId" in list(real_train_df) and "speakerId" in list(synthetic_train_df)
    if have_spk:
        if config.real_speaker_subset_percentage < 1:
            real_train_df = _speaker_subset(real_train_df, config.real_speaker_subset_percentage)
        if config.synthetic_speaker_subset_percentage < 1:
            synthetic_train_df = _speaker_subset(synthetic_train_df, config.synthetic_speaker_subset_percentage)
    else:
        if "speakerId" in list(real_train_df):
            real_train_df = real_train_df.drop(columns="speakerId")
        if "speakerId" in list(synthetic_train_df):
            synthetic_train_df = synthetic_train_df.drop(columns="speakerId")
        for frac in (config.real_speaker_subset_percentage, config.synthetic_speaker_subset_percentage):
            if frac < 1:
                print("no speaker id listed in dataset .csv; ignoring speaker subset selection")
    if config.real_dataset_subset_percentage < 1:
        real_train_df = _select_rows(real_train_df, round(config.real_dataset_subset_percentage * len(real_train_df)))
    if config.synthetic_dataset_subset_percentage < 1:
        synthetic_train_df = _select_rows(
            synthetic_train_df, round(config.synthetic_dataset_subset_percentage * len(synthetic_train_df)))
    train_df = pd.concat([synthetic_train_df, real_train_df]).reset_index()
    valid_df = csv("valid_data.csv")
    test_df = csv("test_data.csv")

    if not config.seq2seq:
        Sy_intent = {"action": {}, "object": {}, "location": {}}
        values_per_slot = []
        for slot in ["action", "object", "location"]:
            slot_values = Counter(train_df[slot])          # first-appearance order, like the reference
            for idx, value in enumerate(slot_values):
                Sy_intent[slot][value] = idx
            values_per_slot.append(len(slot_values))
        config.values_per_slot = values_per_slot
    else:
        # output alphabet: <sos>, every character of the training semantics + string.printable, <eos> (reference
        # data.py:201-208).  The reference orders the characters by iterating a Python set — an order that changes
        # from process to process (string hashing is salted), so its checkpoints only decode within one process;
        # here the set is SORTED: the same alphabet, a reproducible index assignment.
        import string
        chars = set("".join(str(v) for v in train_df["semantics"].tolist()) + string.printable)
        Sy_intent = ["<sos>"] + sorted(chars) + ["<eos>"]
    config.Sy_intent = Sy_intent

    def wordings(path):
        with open(path, "r") as f:
            return [line.strip() for line in f.readlines()]

    if config.train_wording_path is not None:
        train_df = train_df.loc[train_df.transcription.isin(wordings(config.train_wording_path))]
        train_df = train_df.set_index(np.arange(len(train_df)))
    if config.test_wording_path is not None:
        keep = wordings(config.test_wording_path)
        valid_df = valid_df.loc[valid_df.transcription.isin(keep)]
        valid_df = valid_df.set_index(np.arange(len(valid_df)))
        test_df = test_df.loc[test_df.transcription.isin(keep)]
        test_df = test_df.set_index(np.arange(len(test_df)))

    n_ph = _read_phoneme_count(config)
    if n_ph is not None:
        config.num_phonemes = n_ph
    train_dataset = SLUDataset(train_df, base_path, Sy_intent, config, upsample_factor=config.dataset_upsample_factor,
                               shard=True)
    valid_dataset = SLUDataset(valid_df, base_path, Sy_intent, config)
    test_dataset = SLUDataset(test_df, base_path, Sy_intent, config)
    return train_dataset, valid_dataset, test_dataset


def get_ASR_datasets(config):
    """(train, valid, test) ASR pre-training datasets (reference data.py:393-451).  `asr_path` holds
    `text/<split>*/<speaker>/<chapter>/<utt>.TextGrid` alignments and the matching `audio/...wav` files
    (splits train* / dev* / test*), or is `synthetic[:NxBxT]`.  The phoneme / word vocabularies are read
    from <folder>/pretraining/{phonemes,words}.txt or built from the dev split (phonemes in first-seen
    order with stress digits stripped, the `vocabulary_size` most common words) and written there."""
    spec = _synthetic_spec(config.asr_path)
    if spec is not None:
        nb, bs, ns = spec
        bs = bs or config.pretraining_batch_size
        config.num_phonemes = 42
        mk = lambda n, seed: SyntheticASRDataset(n, bs, ns, config, seed=seed)
        rank = _world()[0]
        return (mk(nb, config.seed + 1000003 * rank), mk(max(1, nb // 4), config.seed + 1),
                mk(max(1, nb // 4), config.seed + 2))
    import glob
    base_path = config.asr_path
    wavs = lambda tgs: [p.replace("text", "audio").replace(".TextGrid", ".wav") for p in tgs]
    # sorted: glob returns the directory order of the file system, which differs from machine to machine — and with it the
    # ties of the vocabulary count below, which utterances share a batch under a given seed, and (under data parallelism,
    # where DistributedSampler indexes into the list) which rank gets which file
    if asr_ctc_enabled() and not glob.glob(base_path + "/text/*/*/*/*.TextGrid"):
        return _transcript_datasets(config)              # no alignments: LibriSpeech's own transcripts (CTC only)
    train_tg = sorted(glob.glob(base_path + "/text/train*/*/*/*.TextGrid"))
    valid_tg = sorted(glob.glob(base_path + "/text/dev*/*/*/*.TextGrid"))
    test_tg = sorted(glob.glob(base_path + "/text/test*/*/*/*.TextGrid"))
    ph_file = os.path.join(config.folder, "pretraining", "phonemes.txt")
    wd_file = os.path.join(config.folder, "pretraining", "words.txt")
    rank, world = _world()
    if world > 1:
        # one rank builds the vocabulary files, the others read them
        import torch.distributed as dist
        if rank != 0:
            dist.barrier()
    if os.path.isfile(ph_file) and os.path.isfile(wd_file):
        with open(ph_file, "r") as f:
            Sy_phoneme = [ln.rstrip("\n") for ln in f.readlines() if ln.rstrip("\n") != ""]
        with open(wd_file, "r") as f:
            Sy_word = [ln.rstrip("\n") for ln in f.readlines()]
        config.num_phonemes = len(Sy_phoneme)
    else:
        print("Getting vocabulary...")
        phoneme_counter, word_counter = Counter(), Counter()
        for path in valid_tg:
            tg = read_textgrid(path)
            phoneme_counter.update([_strip_stress(m) for _, _, m in tg["phones"] if m != ""])
            word_counter.update([m for _, _, m in tg["words"]])
        Sy_phoneme = list(phoneme_counter)
        Sy_word = [w[0] for w in word_counter.most_common(config.vocabulary_size)]
        config.num_phonemes = len(Sy_phoneme)
        with open(ph_file, "w") as f:
            for phoneme in Sy_phoneme:
                f.write(phoneme + "\n")
        with open(wd_file, "w") as f:
            for word in Sy_word:
                f.write(word + "\n")
    if world > 1 and rank == 0:
        dist.barrier()
    print("Done.")
    mk = lambda tgs, shard=False: ASRDataset(wavs(tgs), tgs, Sy_phoneme, Sy_word, config, shard=shard)
    return mk(train_tg, True), mk(valid_tg), mk(test_tg)
