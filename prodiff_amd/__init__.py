"""prodiff_amd -- MI355X-native ProDiff mel denoiser/sampler and FastDiff vocoder.

Drop-in replacements for the reference hot path (see DESIGN.md / INTEGRATION.md):
  * prodiff_amd.prodiff.WaveNet            <- modules/decoder/wavenet.py:WaveNet
  * prodiff_amd.prodiff.GaussianDiffusion  <- modules/diffusion/prodiff.py:GaussianDiffusion
  * prodiff_amd.fastdiff.FastDiff          <- modules/FastDiff/module/FastDiff_model.py:FastDiff
  * prodiff_amd.fastdiff.sampling_given_noise_schedule <- modules/FastDiff/module/util.py
  * prodiff_amd.vocoder.FastDiff (registered vocoder) <- component/vocoder/fastdiff.py
  * prodiff_amd.reflow.RectifiedFlow / PitchRectifiedFlow <- modules/diffusion/reflow.py
  * prodiff_amd.teacher.ProDiffTeacher (forward_condition on the GPU)
        <- modules/svs/prodiff_teacher.py:ProDiffTeacher
  * prodiff_amd.variance.PitchPredictor / DurPredictor (encoders and duration head on the GPU)
        <- modules/variance_predictor/pitch_predictor.py, dur_predictor.py
  * prodiff_amd.nsf_hifigan.Generator / NsfHifiGAN (registered vocoder)
        <- modules/nsf_hifigan/models.py, component/vocoder/nsf_hifigan.py
  * prodiff_amd.mel.STFT / mel_filterbank (get_mel on the GPU; NsfHifiGAN.wav2spec)
        <- modules/nsf_hifigan/nvSTFT.py:STFT, librosa.filters.mel
  * prodiff_amd.resample.Resample / resample / KAISER_BEST (polyphase sinc resampler on the GPU)
        <- torchaudio.transforms.Resample (component/pe/rmvpe.py:49), librosa.resample (utils/data_gen_utils.py:51)
  * prodiff_amd.rmvpe.RMVPE / E2E0 / MelSpectrogram / to_local_average_f0 / viterbi_path / to_viterbi_f0 / align_f0
    (pitch extraction on the GPU, up to the f0 curve on the mel frame grid)
        <- component/pe/rmvpe.py, modules/rmvpe/{model,deepunet,seq,spec,utils}.py, librosa.sequence.viterbi,
           utils/pitch_utils.py (interp_f0, resample_align_curve)
  * prodiff_amd.vr.CascadedNet / load_sep_model / extract_harmonic_aperiodic (harmonic-noise separation on the GPU)
        <- modules/vr/{nets,layers,__init__}.py, component/binarizer/binarizer_utils.py
  * prodiff_amd.curves.get_energy / get_voicing / get_breath / get_kth_harmonic / get_tension /
    SinusoidalSmoothingConv1d / VarianceCurves / isolate_parts (variance curves and k-th harmonic isolation on the GPU)
        <- component/binarizer/binarizer_utils.py, modules/commons/common_layers.py, librosa.feature.rms,
           librosa.amplitude_to_db
  * prodiff_amd.analysis.process_utterance / integrated_loudness / normalize_loudness; vocoder.FastDiff.wav2mel /
    wav2wav (FastDiff's analysis half on the GPU: BS.1770 loudness, zero-padded centred STFT, linear mel)
        <- utils/data_gen_utils.py:process_utterance, pyloudnorm.Meter / normalize.loudness, librosa.stft
All compute runs in libprodiff_hip.so (hand-written gfx950 HIP kernels).
"""
from .prodiff import GaussianDiffusion, WaveNet  # noqa: F401
from .fastdiff import FastDiff, sampling_given_noise_schedule  # noqa: F401
from .reflow import PitchRectifiedFlow, RectifiedFlow  # noqa: F401
from .nsf_hifigan import Generator as NsfGenerator, NsfHifiGAN  # noqa: F401
from .teacher import ProDiffTeacher  # noqa: F401
from .variance import DurPredictor, PitchPredictor  # noqa: F401
from .mel import STFT, mel_filterbank  # noqa: F401
# the functional form stays prodiff_amd.resample.resample: binding it here would hide the module of that name
from .resample import KAISER_BEST, Resample, sinc_resample_kernel64  # noqa: F401
from .rmvpe import (E2E0, RMVPE, MelSpectrogram, align_f0, to_local_average_f0, to_viterbi_f0,  # noqa: F401
                    viterbi_path)
from .vr import CascadedNet, extract_harmonic_aperiodic, load_sep_model  # noqa: F401
from .curves import (SinusoidalSmoothingConv1d, VarianceCurves, get_breath, get_energy, get_kth_harmonic,  # noqa: F401
                     get_tension, get_voicing, isolate_parts)
from .analysis import integrated_loudness, normalize_loudness, process_utterance  # noqa: F401

__all__ = ["WaveNet", "GaussianDiffusion", "FastDiff", "sampling_given_noise_schedule", "RectifiedFlow",
           "PitchRectifiedFlow", "NsfGenerator", "NsfHifiGAN", "ProDiffTeacher", "PitchPredictor", "DurPredictor",
           "STFT", "mel_filterbank", "Resample", "KAISER_BEST", "sinc_resample_kernel64", "E2E0", "RMVPE",
           "MelSpectrogram", "to_local_average_f0", "viterbi_path", "to_viterbi_f0", "align_f0", "CascadedNet",
           "load_sep_model", "extract_harmonic_aperiodic", "SinusoidalSmoothingConv1d", "VarianceCurves", "get_energy", "get_voicing", "get_breath", "get_kth_harmonic",
           "get_tension", "isolate_parts", "integrated_loudness", "normalize_loudness", "process_utterance"]
