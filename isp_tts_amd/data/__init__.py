from .features import (AcousticFeatures, collate_audio, melscale_fbanks, pack_filterbank, pitch_frames,  # noqa: F401
                       twiddles, yin_lags)
