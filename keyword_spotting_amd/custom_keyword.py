"""Customised-keyword serving -- the decision of the reference's demo server (server_demo.py:104-130) on a model with two
dense layers (README "Customize keyword": the trained [H, C] head and a second [H, C2] head on the same frozen GRU stack,
"do softmax and decode respectively").

    model = DeployModel(config, weights)          # config.num_classes2 set, weights with Wfc2 / bfc2
    hit, text = predict_ctc(model, pcm, config.label_seqs)

That is the whole-utterance form.  The streaming form -- both heads decoded per chunk in the detector loop, one stack run, a
window per head -- is detector.StreamManager(model, batch, label=..., label2=...) (device) and its host mirror
detector.HotwordDetector(model, label=..., label2=...).
"""
from . import prediction as _prediction
from .rnn_ctc import FEED_INPUT, FEED_STATE, FETCH_NN_OUTPUTS, FETCH_SOFTMAX1, FETCH_SOFTMAX2


def predict_ctc(model, inputX, label_seqs, decoders=_prediction):
    """server_demo.py:104-130.  One utterance `inputX` (what model/inputX:0 takes: 1-D PCM or [T, n_mel] mel) from the zero
    state -> (result, output1, output2): the two decoded [0, w, 0, ...] sequences and result = ctc_predict(output1) |
    ctc_predict(output2).  Head 1 goes through ctc_decode_strict and head 2 through ctc_decode, each called with its own class
    count, positionally as the server does -- which makes it ctc_decode's `lockout` (utils/prediction.py:18), the server's
    behaviour and kept.  `decoders`: the module the three functions come from (keyword_spotting_amd.prediction)."""
    classes1, classes2 = model.config.num_classes, model.num_classes2
    softmax1, softmax2, _ = model.run([FETCH_SOFTMAX1, FETCH_SOFTMAX2, FETCH_NN_OUTPUTS],
                                      {FEED_INPUT: inputX, FEED_STATE: model.zero_state(1)})
    output1 = decoders.ctc_decode_strict(softmax1, classes1)
    output2 = decoders.ctc_decode(softmax2, classes2)
    result = decoders.ctc_predict(output1, label_seqs) | decoders.ctc_predict(output2, label_seqs)
    return result, output1, output2
