"""MI355X-native Silero-VAD v6 inference engine: hand-written HIP kernels for gfx950 behind a
C ABI (include/silero_vad_hip.h), with the reference package's Python surface on top.

    from silero_vad_amd import load_silero_vad, get_speech_timestamps, VADIterator
"""
from .engine import Engine, HipSileroVAD, load_silero_vad  # noqa: F401
from .timestamps import (VADIterator, collect_chunks, drop_chunks, get_speech_timestamps,  # noqa: F401
                         read_audio, read_wav_raw, save_audio, segment_probs)
from .streams import (BatchVADIterator, PackedRecordings, RaggedPlan, RefillPlan, StreamPool, StreamPump, UtteranceCollector, tape_window, tape_run, snapshot_tape, refill_probs, refill_reserve, refill_segments_stream, refill_speech_segments, ragged_buckets, ragged_probs, ragged_reserve,  # noqa: F401
                      ragged_speech_segments, ragged_speech_audio, collect_chunks_device, segment_probs_batch, segment_probs_batch_device, g711_expand, adpcm_expand, decimate, resample, resample_device, resample_geometry, resample_table, resample_stream, resample_stream_ready, resample_stream_history, snapshot_info, ROW_SILENT, deinterleave, channel_rows,
                      ThresholdCounts, ThresholdPairs, LABEL_IGNORE, threshold_pairs, chunk_labels, threshold_counts, threshold_counts_device, ragged_threshold_counts, search_thresholds,
                      ValidationScores, SCORE_KEY_NONE, chunk_scores, chunk_scores_device, ragged_validation, validate)
from .tuning import (DecoderTrainer, decoder_grad, decoder_grad_host, decoder_grad_workspace_bytes, decoder_state_dict, replace_decoder, tune,  # noqa: F401
                     DECODER_NAMES, FusedAdam, TrainingSet, decoder_adam, decoder_adam_host)
from .augment import (Augmenter, RECIPE_DTYPE, augment_device, augment_host, augment_workspace_bytes, biquad_design, check_recipes,  # noqa: F401
                      make_recipes, ALL_TRANSFORMS, augment_scratch_bytes, fir_bank, rir_shoebox)
from .sharding import shard_range, shard_by_duration, gather_to_rank0, batch_speech_timestamps  # noqa: F401

__version__ = "0.1.0"
