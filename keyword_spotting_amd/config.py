"""Model/stream configuration -- the subset of config/rnn_config.py the inference path reads."""


class Config(object):
    """Attribute bag like the reference's (config/rnn_config.py:20-99); defaults are the
    BASELINE north-star shape (n_mel=40 from README.md:17; the repo file ships n_mel=60, :63)."""

    def __init__(self, **overrides):
        self.label_dict = {"ni3": 1, "hao3": 2, "le4": 3}   # :26  0 space, 4 other, 5 ctc blank
        self.label_seqs = "1233"                            # :28
        self.fft_size = 400                                 # :57
        self.hop_size = 160                                 # :58
        self.samplerate = 16000                             # :59
        self.n_mel = 40                                     # :63 (60 in the repo file)
        self.fmin = 300                                     # :64
        self.fmax = 8000                                    # :65
        self.num_layers = 2                                 # :76
        self.use_residual = False                           # :78  ResidualWrapper on layers >= 1 (models/rnn_ctc.py:196-197)
        self.use_layer_norm = False                         # :79  LayerNormalizer around every GRUCell (models/rnn_ctc.py:186-187)
        self.value_clip = -1.0                              # :80
        self.use_relu = False                               # :83
        self.hidden_size = 128                              # :84
        self.precision = "fp32"                             # "fp32" (reference arithmetic) | "f16x3" (fp32 results on the fp16 matrix pipe, split operands) | "bf16" | "int8" (octbit graph) -- BASELINE configs[2]
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise AttributeError("unknown config key %r" % k)
            setattr(self, k, type(getattr(self, k))(v) if not isinstance(getattr(self, k), dict) else v)

    @property
    def num_classes(self):                                  # :88-91
        return len(self.label_dict) + 3

    @property
    def freq_size(self):                                    # :97-99 (mfcc=False)
        return self.n_mel


def get_config(**overrides):
    return Config(**overrides)


class AttentionConfig(Config):
    """The fields of config/attention_config.py the self-attention CTC model's inference reads (its defaults: n_mel 60 :67,
    use_relu :55, combine_frame :79, num_layers :80, feed_forward_inner_size :82, multi_head_num :84, hidden_size :85), and
    max_frames: the longest utterance (mel frames) a DeployModel takes -- the size of its positional table.
    mfcc=True switches the in-graph front-end to utils/mfcc.py (models/attention_ctc.py:249-250): the model's input width
    freq_size becomes 3 * n_mfcc."""

    def __init__(self, **overrides):
        self.label_dict = {"ni3": 1, "hao3": 2, "le4": 3}   # :26-27
        self.label_seqs = "1233"                            # :28
        self.fft_size = 400                                 # :59
        self.hop_size = 160                                 # :60
        self.samplerate = 16000                             # :61
        self.mfcc = False                                   # :23
        self.power = 1                                      # :63  (the deploy graph never reads it: |rfft|, or |rfft|^2 inside mfcc())
        self.n_mel = 60                                     # :67
        self.n_mfcc = 20                                    # :66
        self.pre_emphasis = False                           # :68  process_wav.py:72-73, in front of the dataset's STFT (DatasetFrontend)
        self.fmin = 300                                     # :64
        self.fmax = 8000                                    # :65
        self.use_relu = True                                # :55
        self.combine_frame = 2                              # :79
        self.num_layers = 3                                 # :80
        self.feed_forward_inner_size = 512                  # :82
        self.multi_head_num = 8                             # :84
        self.hidden_size = 128                              # :85
        self.max_frames = 8192                              # not in the reference: the positional table's extent
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise AttributeError("unknown config key %r" % k)
            setattr(self, k, type(getattr(self, k))(v) if not isinstance(getattr(self, k), dict) else v)

    @property
    def freq_size(self):                                    # :97-99
        return self.n_mfcc * 3 if self.mfcc else self.n_mel


def get_attention_config(**overrides):
    return AttentionConfig(**overrides)
