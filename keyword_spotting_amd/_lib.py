"""ctypes binding of libkws_amd.so (include/kws_amd.h).  Fails loudly when the library is missing."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KWS_AMD_LIB", os.path.join(_HERE, "libkws_amd.so"))   # override: timing experiments

KWS_OK = 0
KWS_ERR_INVALID_ARGUMENT = -1
KWS_ERR_UNSUPPORTED = -2
KWS_ERR_HIP = -3
KWS_ERR_NO_DEVICE = -4
KWS_ERR_OUT_OF_MEMORY = -5
KWS_ERR_BUSY = -6
KERNEL_AUTO, KERNEL_GENERIC, KERNEL_RESIDENT = 0, 1, 2
DECODE, DECODE2, DECODE_STRICT = 0, 1, 2
FP32, BF16, INT8, F16X3 = 0, 1, 2, 3
FEAT_MEL, FEAT_MFCC = 0, 1
FRAMES_DEPLOY, FRAMES_DATASET = 0, 1
OPT_ADAM, OPT_NESTEROV = 0, 1


class KwsConfig(ctypes.Structure):
    _fields_ = [("n_mel", ctypes.c_int32), ("hidden", ctypes.c_int32), ("num_layers", ctypes.c_int32),
                ("num_classes", ctypes.c_int32), ("use_relu", ctypes.c_int32),
                ("value_clip", ctypes.c_float), ("precision", ctypes.c_int32)]


class KwsFrontendConfig(ctypes.Structure):
    _fields_ = [("samplerate", ctypes.c_int32), ("fft_size", ctypes.c_int32), ("hop_size", ctypes.c_int32),
                ("n_mel", ctypes.c_int32), ("fmin", ctypes.c_float), ("fmax", ctypes.c_float)]


class KwsFeatureConfig(ctypes.Structure):
    """kws_feature_config: what a front-end handle produces (mel of |X| or |X|^2, or MFCC + deltas, utils/mfcc.py)."""
    _fields_ = [("base", KwsFrontendConfig), ("kind", ctypes.c_int32), ("power", ctypes.c_int32), ("n_mfcc", ctypes.c_int32)]


class KwsDatasetConfig(ctypes.Structure):
    """kws_dataset_config: a feature front-end and how it frames the utterance -- as the deploy graph, or as the dataset's
    librosa.stft (centred, reflect-padded, Hann-windowed) behind an optional pre-emphasis (process_wav.py:38-44,69-78)."""
    _fields_ = [("feat", KwsFeatureConfig), ("framing", ctypes.c_int32), ("pre_emphasis", ctypes.c_float)]


class KwsCellWrappers(ctypes.Structure):
    """kws_cell_wrappers: the reference's get_cell options (config/rnn_config.py:78-79), 0 or 1 each."""
    _fields_ = [("use_layer_norm", ctypes.c_int32), ("use_residual", ctypes.c_int32)]


class KwsTrainConfig(ctypes.Structure):
    """kws_train_config: the model, the options a train handle refuses (wrappers, variational_recurrent), the optimiser, the global-norm
    clip (<= 0: none) and the output keep probability of the dropout masks."""
    _fields_ = [("model", KwsConfig), ("wrappers", KwsCellWrappers), ("variational_recurrent", ctypes.c_int32),
                ("optimizer", ctypes.c_int32), ("max_grad_norm", ctypes.c_float), ("keep_prob", ctypes.c_float)]


class KwsTrainStateIo(ctypes.Structure):
    """kws_train_state_io: the carried states of a kws_train_grad_state / kws_train_step_state call, [L,B,H] f32 device pointers, 16-byte
    aligned, each may be NULL -- state_in (NULL: zeros), state_out, dstate_out (NULL: zeros), dstate_in."""
    _fields_ = [("state_in", ctypes.c_void_p), ("state_out", ctypes.c_void_p), ("dstate_out", ctypes.c_void_p), ("dstate_in", ctypes.c_void_p)]


class KwsFrameTargets(ctypes.Structure):
    """kws_frame_targets: the frame-wise targets of a kws_[attention_]train_*_frames call -- targets [B,T] int32 (device; -1: no target),
    class_weight [C] f32 (host) or NULL, the two weights of loss[b] = ctc_weight ctc_b + frame_weight ce_b, and frame_loss [B] (device
    out) or NULL for ce_b alone."""
    _fields_ = [("targets", ctypes.c_void_p), ("class_weight", ctypes.c_void_p), ("ctc_weight", ctypes.c_float),
                ("frame_weight", ctypes.c_float), ("frame_loss", ctypes.c_void_p)]


class KwsHeadIo(ctypes.Structure):
    """kws_head_io: one class head's outputs in kws_step_heads -- logits / softmax [B,T,C_i], tokens [B,T], prev_word [B] (device
    pointers, each may be NULL; tokens needs prev_word) and the head's ctc_decode2 threshold."""
    _fields_ = [("logits", ctypes.c_void_p), ("softmax", ctypes.c_void_p), ("tokens", ctypes.c_void_p),
                ("prev_word", ctypes.c_void_p), ("decode2_thres", ctypes.c_float)]


class KwsAttentionConfig(ctypes.Structure):
    """kws_attention_config: the self-attention CTC model (config/attention_config.py) and the longest utterance a handle takes."""
    _fields_ = [("n_mel", ctypes.c_int32), ("combine_frame", ctypes.c_int32), ("hidden", ctypes.c_int32),
                ("num_heads", ctypes.c_int32), ("ffn_inner", ctypes.c_int32), ("num_layers", ctypes.c_int32),
                ("num_classes", ctypes.c_int32), ("use_relu", ctypes.c_int32), ("max_frames", ctypes.c_int32)]


class KwsAttentionTrainConfig(ctypes.Structure):
    """kws_attention_train_config: the attention model, the optimiser, the global-norm clip (<= 0: none) and the keep probability of the
    three dropout sites."""
    _fields_ = [("model", KwsAttentionConfig), ("optimizer", ctypes.c_int32), ("max_grad_norm", ctypes.c_float), ("keep_prob", ctypes.c_float)]


class KwsError(RuntimeError):
    """Base of the errors the C ABI reports."""

    def __init__(self, code, msg):
        RuntimeError.__init__(self, "kws_amd error %d: %s" % (code, msg))
        self.code = code


class InvalidArgumentError(KwsError, ValueError):
    """Mirror of tf.errors.InvalidArgumentError on the reference's boundary."""


class UnsupportedError(KwsError, NotImplementedError):
    pass


class BusyError(KwsError):
    """Another host thread is inside a call on the same handle (one thread at a time per handle)."""


_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_SIGNATURES = {
    "kws_version": (ctypes.c_char_p, []),
    "kws_last_error": (ctypes.c_char_p, []),
    "kws_sizeof_config": (ctypes.c_size_t, []),
    "kws_sizeof_frontend_config": (ctypes.c_size_t, []),
    "kws_weights_nbytes": (ctypes.c_size_t, [ctypes.POINTER(KwsConfig)]),
    "kws_create": (_i, [ctypes.POINTER(KwsConfig), _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kws_sizeof_cell_wrappers": (ctypes.c_size_t, []),
    "kws_weights_nbytes_wrapped": (ctypes.c_size_t, [ctypes.POINTER(KwsConfig), ctypes.POINTER(KwsCellWrappers)]),
    "kws_create_wrapped": (_i, [ctypes.POINTER(KwsConfig), ctypes.POINTER(KwsCellWrappers), _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kws_sizeof_head_io": (ctypes.c_size_t, []),
    "kws_weights_nbytes_heads": (ctypes.c_size_t, [ctypes.POINTER(KwsConfig), ctypes.c_int32]),
    "kws_create_heads": (_i, [ctypes.POINTER(KwsConfig), ctypes.c_int32, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kws_step_heads": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(KwsHeadIo), ctypes.POINTER(KwsHeadIo), _i, _i, _vp]),
    "kws_destroy": (_i, [_vp]),
    "kws_set_kernel": (_i, [_vp, _i]),
    "kws_reserve": (_i, [_vp, _i, _i]),
    "kws_scratch_stats": (_i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]),
    "kws_poll_error": (_i, [_vp]),
    "kws_selftest": (_i, [_vp]),
    "kws_last_launch": (_i, [_vp, _i, ctypes.c_char_p, ctypes.c_size_t]),
    "kws_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i, _i, _vp]),
    "kws_set_profiling": (_i, [_vp, _i]),
    "kws_kernel_times": (_i, [_vp, _vp, _vp, _i]),
    "kws_ctc_decode": (_i, [_i, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _i, _vp]),
    "kws_ctc_predict": (_i, [_vp, _vp, _i, _i, ctypes.c_char_p, _vp, _vp]),
    "kws_vad": (_i, [_vp, _i, _i, _f, _vp, _vp, _vp]),
    "kws_frontend_create": (_i, [ctypes.POINTER(KwsFrontendConfig), ctypes.POINTER(_vp)]),
    "kws_frontend_destroy": (_i, [_vp]),
    "kws_frontend_frames": (_i, [ctypes.POINTER(KwsFrontendConfig), _i]),
    "kws_frontend_run": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "kws_frontend_run_carry": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    "kws_frontend_mel_basis": (_i, [_vp, _vp]),
    "kws_sizeof_feature_config": (ctypes.c_size_t, []),
    "kws_frontend_create_features": (_i, [ctypes.POINTER(KwsFeatureConfig), ctypes.POINTER(_vp)]),
    "kws_frontend_feature_size": (_i, [_vp]),
    "kws_frontend_run_lengths": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "kws_frontend_dct_basis": (_i, [_vp, _vp]),
    "kws_sizeof_dataset_config": (ctypes.c_size_t, []),
    "kws_frontend_create_dataset": (_i, [ctypes.POINTER(KwsDatasetConfig), ctypes.POINTER(_vp)]),
    "kws_frontend_frames_of": (_i, [_vp, _i]),
    "kws_frontend_window": (_i, [_vp, _vp]),
    # the reader's noise augmentation: the linear spectrum as an output, and the mix in front of the feature epilogues
    "kws_frontend_linear_size": (_i, [_vp]),
    "kws_frontend_run_linear": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "kws_frontend_augment": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "kws_window_create": (_i, [_i, _i, _i, _i, _f, ctypes.POINTER(_vp)]),
    "kws_window_destroy": (_i, [_vp]),
    "kws_window_step": (_i, [_vp, _vp, _i, _vp, ctypes.c_char_p, _vp, _vp, _vp]),
    "kws_window_step_incremental": (_i, [_vp, _vp, _i, _vp, ctypes.c_char_p, _vp, _vp, _vp]),
    "kws_stream_create": (_i, [_vp, _vp, _vp, _i, _i, _f, ctypes.c_char_p, _vp, _vp, ctypes.POINTER(_vp)]),
    "kws_stream_create_heads": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, ctypes.c_char_p, ctypes.c_char_p, _vp, _vp, ctypes.POINTER(_vp)]),
    "kws_step_heads_window": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, ctypes.c_char_p, ctypes.c_char_p, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kws_stream_destroy": (_i, [_vp]),
    "kws_stream_reset": (_i, [_vp]),
    "kws_stream_feed": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "kws_stream_feed_ragged": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "kws_stream_recycle": (_i, [_vp, _vp, _vp]),
    "kws_stream_carry": (_i, [_vp, _vp, _vp, _vp]),
    "kws_octbit_matmul": (_i, [_vp, _vp, _f, _vp, _vp, _i, _i, _i, _i, _vp]),
    "kws_octbit_quantize": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "kws_sizeof_attention_config": (ctypes.c_size_t, []),
    "kws_attention_weights_nbytes": (ctypes.c_size_t, [ctypes.POINTER(KwsAttentionConfig)]),
    "kws_attention_create": (_i, [ctypes.POINTER(KwsAttentionConfig), _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kws_attention_create_precision": (_i, [ctypes.POINTER(KwsAttentionConfig), _i, _vp, ctypes.c_size_t, ctypes.POINTER(_vp)]),
    "kws_attention_destroy": (_i, [_vp]),
    "kws_attention_frames_out": (_i, [ctypes.POINTER(KwsAttentionConfig), _i]),
    "kws_attention_reserve": (_i, [_vp, _i, _i]),
    "kws_attention_run": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "kws_attention_pe_table": (_i, [_vp, _vp]),
    "kws_attention_selftest": (_i, [_vp]),
    # the self-attention model on live streams: the sliding-window manager
    "kws_attention_stream_create": (_i, [_vp, _vp, _i, _i, _i, _f, _f, ctypes.c_char_p, ctypes.POINTER(_vp)]),
    "kws_attention_stream_destroy": (_i, [_vp]),
    "kws_attention_stream_feed": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "kws_attention_stream_recycle": (_i, [_vp, _vp, _vp]),
    "kws_attention_stream_window": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "kws_attention_stream_carry": (_i, [_vp, _vp, _vp, _vp]),
    "kws_attention_stream_stats": (_i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32)]),
    "kws_ctc_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "kws_ctc_beam_search": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "kws_ctc_align": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "kws_enroll_create": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_vp)]),
    "kws_enroll_destroy": (_i, [_vp]),
    "kws_enroll_set": (_i, [_vp, _vp, _vp, _vp]),
    "kws_enroll_fit": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp]),
    "kws_enroll_fit_frames": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, ctypes.POINTER(KwsFrameTargets), _f, _i, _vp, _vp]),
    "kws_enroll_check_frames": (_i, [_i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, ctypes.POINTER(KwsFrameTargets), _f, _i]),
    "kws_enroll_get": (_i, [_vp, _vp, _vp, _vp]),
    "kws_enroll_moments": (_i, [_vp, _vp, _vp, _vp]),
    "kws_enroll_stats": (_i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    # training of the stack: taped forward, BPTT, CTC loss, clip, Adam / Nesterov
    "kws_sizeof_train_config": (ctypes.c_size_t, []),
    "kws_train_create": (_i, [ctypes.POINTER(KwsTrainConfig), ctypes.POINTER(_vp)]),
    "kws_train_check": (_i, [ctypes.POINTER(KwsTrainConfig), _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kws_train_create_wrapped": (_i, [ctypes.POINTER(KwsTrainConfig), ctypes.POINTER(_vp)]),
    "kws_train_check_wrapped": (_i, [ctypes.POINTER(KwsTrainConfig), _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kws_train_destroy": (_i, [_vp]),
    "kws_train_set_weights": (_i, [_vp, _vp, ctypes.c_size_t, _vp]),
    "kws_train_get_weights": (_i, [_vp, _vp, ctypes.c_size_t, _vp]),
    "kws_train_reserve": (_i, [_vp, _i, _i, _i]),
    "kws_train_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "kws_train_step": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _vp, _vp, _vp]),
    "kws_train_moments": (_i, [_vp, _vp, _vp, _vp]),
    "kws_train_stats": (_i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                             ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    # ... from and to carried states, and the optimiser step from a gradient the caller supplies
    "kws_sizeof_train_state_io": (ctypes.c_size_t, []),
    "kws_train_grad_state": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(KwsTrainStateIo), _vp]),
    "kws_train_step_state": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _vp, _vp, ctypes.POINTER(KwsTrainStateIo), _vp]),
    "kws_train_check_state": (_i, [ctypes.POINTER(KwsTrainConfig), _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, ctypes.POINTER(KwsTrainStateIo)]),
    "kws_train_apply": (_i, [_vp, _vp, _f, _vp, _vp]),
    # training of the self-attention CTC model: taped forward, backward, CTC loss, clip, Adam / Nesterov; the dropout hash on the host
    "kws_sizeof_attention_train_config": (ctypes.c_size_t, []),
    "kws_attention_train_create": (_i, [ctypes.POINTER(KwsAttentionTrainConfig), ctypes.POINTER(_vp)]),
    "kws_attention_train_check": (_i, [ctypes.POINTER(KwsAttentionTrainConfig), _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "kws_attention_train_destroy": (_i, [_vp]),
    "kws_attention_train_set_weights": (_i, [_vp, _vp, ctypes.c_size_t, _vp]),
    "kws_attention_train_get_weights": (_i, [_vp, _vp, ctypes.c_size_t, _vp]),
    "kws_attention_train_reserve": (_i, [_vp, _i, _i, _i]),
    "kws_attention_train_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    "kws_attention_train_step": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.c_uint64, _f, _vp, _vp, _vp]),
    "kws_attention_train_moments": (_i, [_vp, _vp, _vp, _vp]),
    "kws_attention_train_stats": (_i, [_vp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]),
    "kws_attention_drop_keep": (_i, [ctypes.c_uint64, _f, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    # frame-wise targets: the cross-entropy as an op, and as the loss (alone or mixed with the CTC loss) of both train handles
    "kws_frame_loss": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "kws_sizeof_frame_targets": (ctypes.c_size_t, []),
    "kws_train_grad_frames": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, ctypes.POINTER(KwsTrainStateIo),
                                   ctypes.POINTER(KwsFrameTargets), _vp]),
    "kws_train_step_frames": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _f, _vp, _vp, ctypes.POINTER(KwsTrainStateIo),
                                   ctypes.POINTER(KwsFrameTargets), _vp]),
    "kws_train_check_frames": (_i, [ctypes.POINTER(KwsTrainConfig), _i, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, ctypes.POINTER(KwsTrainStateIo),
                                    ctypes.POINTER(KwsFrameTargets)]),
    "kws_attention_train_grad_frames": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.c_uint64, _vp, _vp, _vp,
                                             ctypes.POINTER(KwsFrameTargets), _vp]),
    "kws_attention_train_step_frames": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, ctypes.c_uint64, _f, _vp, _vp,
                                             ctypes.POINTER(KwsFrameTargets), _vp]),
    "kws_attention_train_check_frames": (_i, [ctypes.POINTER(KwsAttentionTrainConfig), _vp, _vp, _vp, _vp, _i, _i, _i, _vp,
                                              ctypes.POINTER(KwsFrameTargets)]),
    # a bank of enrolled heads: per-user customised keywords on one frozen model
    "kws_bank_create": (_i, [_i, _i, _i, _i, ctypes.POINTER(_vp)]),
    "kws_bank_destroy": (_i, [_vp]),
    "kws_bank_set": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "kws_bank_get": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "kws_bank_set_keyword": (_i, [_vp, _i, _i, ctypes.c_char_p, _vp]),
    "kws_bank_get_keyword": (_i, [_vp, _i, ctypes.POINTER(_i), ctypes.c_char_p, ctypes.POINTER(_i)]),
    "kws_step_bank": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(KwsHeadIo), ctypes.POINTER(KwsHeadIo), _i, _i, _vp]),
    "kws_stream_create_bank": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, ctypes.c_char_p, ctypes.c_char_p, _vp, _vp, ctypes.POINTER(_vp)]),
    "kws_step_bank_window": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, ctypes.c_char_p, ctypes.c_char_p, _vp, _vp, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(sorted(_SIGNATURES))

_lib = None


def load():
    """Returns the loaded library; raises ImportError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing -- build it with `make -C keyword_spotting_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime of this process BEFORE
        # libkws_amd.so resolves its libamdhip64 dependency, or the two would not share devices,
        # streams and allocations (a second runtime instance sees "no HIP device").
        import torch  # noqa: F401
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.kws_sizeof_config() != ctypes.sizeof(KwsConfig) or \
                lib.kws_sizeof_frontend_config() != ctypes.sizeof(KwsFrontendConfig) or \
                lib.kws_sizeof_cell_wrappers() != ctypes.sizeof(KwsCellWrappers) or \
                lib.kws_sizeof_feature_config() != ctypes.sizeof(KwsFeatureConfig) or \
                lib.kws_sizeof_dataset_config() != ctypes.sizeof(KwsDatasetConfig) or \
                lib.kws_sizeof_attention_config() != ctypes.sizeof(KwsAttentionConfig) or \
                lib.kws_sizeof_train_config() != ctypes.sizeof(KwsTrainConfig) or \
                lib.kws_sizeof_train_state_io() != ctypes.sizeof(KwsTrainStateIo) or \
                lib.kws_sizeof_attention_train_config() != ctypes.sizeof(KwsAttentionTrainConfig) or \
                lib.kws_sizeof_frame_targets() != ctypes.sizeof(KwsFrameTargets) or \
                lib.kws_sizeof_head_io() != ctypes.sizeof(KwsHeadIo):
            raise ImportError("%s was built from a different include/kws_amd.h than this binding (struct sizes differ); "
                              "rebuild it" % LIB_PATH)
        _lib = lib
    return _lib


def check(rc):
    if rc == KWS_OK:
        return
    msg = load().kws_last_error().decode("utf-8", "replace")
    if rc == KWS_ERR_INVALID_ARGUMENT:
        raise InvalidArgumentError(rc, msg)
    if rc == KWS_ERR_UNSUPPORTED:
        raise UnsupportedError(rc, msg)
    if rc == KWS_ERR_BUSY:
        raise BusyError(rc, msg)
    raise KwsError(rc, msg)


def current_stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
