//! Batch boundary scoring on an AMD MI355X behind the names of `vaporetto::Predictor`.
//!
//! `ffi` declares every entry point of `include/vaporetto_hip.h` (generated from the header by `bindings/rust/gen_ffi.py`;
//! `tests/test_rust_binding.py` in the MI355X repository compares the two, function by function, arity and widths).  This file
//! is the safe layer an application links against without touching the `vaporetto` crate: the model goes in as
//! `Model::to_vec()` bytes (model.rs:99-104), sentences come in as `vaporetto::Sentence`s, labels go back through
//! `Sentence::boundaries_mut()` (sentence.rs:1034) -- so `iter_tokens` / `write_tokenized_text` work on them as after
//! `Predictor::predict` (predictor.rs:518-543) -- and the i32 scores are returned beside them, because a `Sentence`'s score
//! buffer is `pub(crate)` (sentence.rs:92-94).  What needs crate-private access -- scores INSIDE the sentence, tags as
//! `Cow<'b, str>` borrowed from the model (predictor.rs:546-637; `TagModel::tags` is `pub(crate)`, model.rs:41-47) -- is the
//! in-crate variant of this shim, `vaporetto/src/hip.rs` behind a cargo feature, shown in INTEGRATION.md section 2.
//!
//! There is no CPU fallback: without a HIP device every call returns `HipError::Device`; keep the stock `Predictor` for that.
pub mod ffi;

use std::ffi::CStr;
use std::fmt;
use std::os::raw::c_int;

use vaporetto::{CharacterBoundary, Model, Sentence};

/// `VaporettoError`'s kinds (errors.rs:15-38) plus the device.
#[derive(Debug, Clone, PartialEq, Eq)]
pub enum HipError {
    InvalidModel(String),
    InvalidArgument(String),
    Device(String),
}

impl fmt::Display for HipError {
    fn fmt(&self, f: &mut fmt::Formatter) -> fmt::Result {
        match self {
            HipError::InvalidModel(m) | HipError::InvalidArgument(m) | HipError::Device(m) => f.write_str(m),
        }
    }
}
impl std::error::Error for HipError {}

pub type Result<T> = std::result::Result<T, HipError>;

fn check(st: c_int) -> Result<()> {
    if st == ffi::VPT_OK {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(ffi::vpt_last_error()) }.to_string_lossy().into_owned();
    Err(match st {
        ffi::VPT_INVALID_MODEL => HipError::InvalidModel(msg),
        ffi::VPT_INVALID_ARGUMENT => HipError::InvalidArgument(msg),
        _ => HipError::Device(msg),
    })
}

/// `KyteaFullwidthFilter` before scoring, `KyteaWsConstFilter(t)` / `SplitLinebreaksFilter` on the labels (predict/src/main.rs:126-134).
/// `ConcatGraphemeClustersFilter` (`--wsconst G`, predict/src/main.rs:101-104) is `FLAG_CONCAT_GRAPHEMES`: a launch behind the scoring
/// launch that always runs after the other label filters; `concat_graphemes` applies it to labels of the caller's for any other order.
pub const FLAG_KYTEA_FULLWIDTH: u32 = 1;
pub const FLAG_SPLIT_LINEBREAKS: u32 = 1 << 7;
/// With `FLAG_SPLIT_LINEBREAKS`: that filter runs before the wsconst ones (the order of vaporetto_tantivy's post-filters).
pub const FLAG_LINEBREAKS_FIRST: u32 = 1 << 8;
/// `ConcatGraphemeClustersFilter` on the device, after every other label filter (also a bit of `token_stream_batch`'s `wsconst_flags`: the adapter's G).
pub const FLAG_CONCAT_GRAPHEMES: u32 = 1 << 9;
pub const fn flag_wsconst(char_type: u8) -> u32 {
    1 << char_type
}

/// `vpt_train_params.flags` for `ffi::vpt_trainer_create` (include/vaporetto_hip.h, Trainer): tag models; solver 5; solver 5 for the tag
/// models (needs the two before it); solver 6; solver 6 for the tag models (needs `TRAIN_TAGS` and `TRAIN_L1R_LR`).
pub const TRAIN_TAGS: u32 = 1;
pub const TRAIN_L1R: u32 = 4;
pub const TRAIN_TAGS_L1R: u32 = 8;
pub const TRAIN_L1R_LR: u32 = 16;
pub const TRAIN_TAGS_L1R_LR: u32 = 32;

/// `vaporetto::Predictor` for batches, on one GPU.
pub struct HipPredictor {
    raw: *mut ffi::vpt_predictor,
}
// immutable after creation; `&self` calls take a workspace of their own from the library's pool (the header's conventions) --
// what `Arc<Predictor>` is to vaporetto_tantivy/src/lib.rs:62-67
unsafe impl Send for HipPredictor {}
unsafe impl Sync for HipPredictor {}

impl HipPredictor {
    /// `Predictor::new(model, predict_tags)` (predictor.rs:450-508); the model by value, like the reference.
    pub fn new(model: Model, predict_tags: bool, device_id: i32) -> Result<Self> {
        let bytes = model.to_vec().map_err(|e| HipError::InvalidModel(e.to_string()))?;
        Self::from_model_bytes(&bytes, predict_tags, device_id)
    }

    /// The same from `Model::write`'s bytes ("VaporettoTokenizer 0.5.0\n" + bincode; zstd is outside the API, README.md:50-63).
    pub fn from_model_bytes(bytes: &[u8], predict_tags: bool, device_id: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::vpt_predictor_create(bytes.as_ptr(), bytes.len(), predict_tags as c_int, device_id, &mut raw) })?;
        Ok(Self { raw })
    }

    /// `Predictor::predict` over many sentences in one launch: every sentence's `boundaries_mut()` receives its labels; the
    /// i32 scores (`Sentence::boundary_scores()` in the reference, sentence.rs:1040-1046) come back per sentence.
    pub fn predict_batch(&self, sentences: &mut [Sentence<'_, '_>], flags: u32) -> Result<Vec<Vec<i32>>> {
        let (utf8, boff) = pack(sentences.iter().map(|s| s.as_raw_text()));
        let n = sentences.len();
        let mut ooff = vec![0u64; n + 1];
        check(unsafe { ffi::vpt_count_boundaries(utf8.as_ptr(), boff.as_ptr(), n, ooff.as_mut_ptr()) })?;
        let total = ooff[n] as usize;
        let (mut scores, mut labels) = (vec![0i32; total.max(1)], vec![0u8; total.max(1)]);
        check(unsafe {
            ffi::vpt_predict_batch_flags(self.raw, utf8.as_ptr(), boff.as_ptr(), n, scores.as_mut_ptr(), labels.as_mut_ptr(), ooff.as_ptr(), flags)
        })?;
        let mut out = Vec::with_capacity(n);
        for (i, s) in sentences.iter_mut().enumerate() {
            let (a, b) = (ooff[i] as usize, ooff[i + 1] as usize);
            for (dst, &l) in s.boundaries_mut().iter_mut().zip(&labels[a..b]) {
                *dst = if l == 1 { CharacterBoundary::WordBoundary } else { CharacterBoundary::NotWordBoundary };
            }
            out.push(scores[a..b].to_vec());
        }
        Ok(out)
    }

    /// The CLI's per-line loop for a batch of lines (predict/src/main.rs:122-176): `Sentence::from_raw`, the filters as flags,
    /// `predict`, `fill_tags` when `tagged`, `write_tokenized_text` -- only text crosses PCIe.  Returns one tokenized line per input.
    pub fn tokenize_lines<'a, I: IntoIterator<Item = &'a str>>(&self, lines: I, flags: u32, tagged: bool) -> Result<Vec<String>> {
        let (utf8, boff) = pack(lines.into_iter());
        let n = boff.len() - 1;
        let mut suffix = 0u32;
        if tagged {
            check(unsafe { ffi::vpt_predictor_max_tag_suffix(self.raw, &mut suffix) })?;
        }
        let cap = 3 * utf8.len() + 64 + utf8.len() * suffix as usize;
        let mut text = vec![0u8; cap];
        let mut toff = vec![0u64; n + 1];
        check(unsafe {
            ffi::vpt_tokenize_batch(self.raw, utf8.as_ptr(), boff.as_ptr(), n, flags, tagged as c_int, text.as_mut_ptr(), cap as u64, toff.as_mut_ptr())
        })?;
        Ok((0..n).map(|i| String::from_utf8_lossy(&text[toff[i] as usize..toff[i + 1] as usize]).into_owned()).collect())
    }

    /// `VaporettoTokenizer::token_stream` (vaporetto_tantivy/src/lib.rs:160-192) for a batch of documents: `utf8[boff[i] .. boff[i + 1]]` is document i
    /// (empty ones are allowed), `wsconst_flags` the `flag_wsconst` bits of the adapter's D R H T K O and `FLAG_CONCAT_GRAPHEMES` for its G.  Returns `(token_offsets, token_ends)`: document i
    /// owns `token_ends[token_offsets[i] .. token_offsets[i + 1]]`, the byte offset behind every one of its tokens from its first byte (the adapter's
    /// `boundary_pos`).  The C side trusts the sizes, so they are checked here.
    pub fn token_stream_batch(&self, utf8: &[u8], boff: &[u64], wsconst_flags: u32) -> Result<(Vec<u64>, Vec<u32>)> {
        let bad = |what: &str| Err(HipError::InvalidArgument(format!("InvalidArgumentError: {}", what)));
        if boff.is_empty() { return bad("byte_offsets: n + 1 entries"); }
        let n = boff.len() - 1;
        if boff.windows(2).any(|w| w[1] < w[0]) { return bad("offsets: must not decrease"); }
        if (utf8.len() as u64) < boff[n] { return bad("utf8: shorter than byte_offsets[n]"); }
        let capacity = (boff[n] - boff[0]) as usize;   // a token per char at most, a char per byte at most
        let mut offsets = vec![0u64; n + 1];
        let mut ends = vec![0u32; capacity.max(1)];
        check(unsafe {
            ffi::vpt_token_stream_batch(self.raw, utf8.as_ptr(), boff.as_ptr(), n, wsconst_flags, offsets.as_mut_ptr(), ends.as_mut_ptr(), capacity as u64)
        })?;
        ends.truncate(offsets[n] as usize);
        Ok((offsets, ends))
    }

    /// `ConcatGraphemeClustersFilter` on labels of the caller's (`labels[ooff[i] + b]`: boundary b of sentence i, `ooff` from
    /// `vpt_count_boundaries`), in place, on the device; `fullwidth`: the clusters of the `KyteaFullwidthFilter` image.  The sizes are checked here.
    pub fn concat_graphemes(&self, utf8: &[u8], boff: &[u64], ooff: &[u64], fullwidth: bool, labels: &mut [u8]) -> Result<()> {
        let bad = |what: &str| Err(HipError::InvalidArgument(format!("InvalidArgumentError: {}", what)));
        if boff.is_empty() || ooff.len() != boff.len() { return bad("offsets: n + 1 entries each"); }
        let n = boff.len() - 1;
        if boff.windows(2).any(|w| w[1] < w[0]) || ooff.windows(2).any(|w| w[1] < w[0]) { return bad("offsets: must not decrease"); }
        if (utf8.len() as u64) < boff[n] { return bad("utf8: shorter than byte_offsets[n]"); }
        if (labels.len() as u64) < ooff[n] { return bad("labels: shorter than out_offsets[n]"); }
        check(unsafe {
            ffi::vpt_concat_graphemes_batch(self.raw, utf8.as_ptr(), boff.as_ptr(), n, ooff.as_ptr(), if fullwidth { FLAG_KYTEA_FULLWIDTH } else { 0 }, labels.as_mut_ptr())
        })
    }

    /// `Predictor::serialize_to_vec` / `deserialize_from_slice_unchecked` (predictor.rs:640-664), in this library's own format
    /// (version and checksums checked): skips the table compile.
    pub fn serialize_to_vec(&self) -> Result<Vec<u8>> {
        let mut need = 0usize;
        check(unsafe { ffi::vpt_predictor_save(self.raw, std::ptr::null_mut(), 0, &mut need) })?;
        let mut buf = vec![0u8; need];
        check(unsafe { ffi::vpt_predictor_save(self.raw, buf.as_mut_ptr(), buf.len(), &mut need) })?;
        Ok(buf)
    }
    pub fn deserialize_from_slice(blob: &[u8], device_id: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::vpt_predictor_load(blob.as_ptr(), blob.len(), device_id, &mut raw) })?;
        Ok(Self { raw })
    }
    /// The same predictor on another GPU of the node: the tables are copied device to device, nothing is compiled again.
    pub fn clone_to_device(&self, device_id: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::vpt_predictor_clone_to_device(self.raw, device_id, &mut raw) })?;
        Ok(Self { raw })
    }
    pub fn info(&self) -> Result<ffi::vpt_model_info> {
        let mut info = ffi::vpt_model_info::default();
        check(unsafe { ffi::vpt_predictor_info(self.raw, &mut info) })?;
        Ok(info)
    }
}

impl Drop for HipPredictor {
    fn drop(&mut self) {
        unsafe { ffi::vpt_predictor_destroy(self.raw) }
    }
}

/// `vaporetto_rules::sentence_filters::PatternMatchTagger` (pattern_match_tagger.rs:10-41) on the device: `rules[surface]` fills the tag slots
/// `fill_tags` left `None` -- never one that is `Some`; entries past the predictor's `n_tags` are ignored; `None` stays `None`, `Some("")` is a
/// tag.  The table is built on the host and uploaded once, for ONE predictor (its device, its `n_tags`), which it borrows: the predictor
/// outlives the tagger.  `HipPredictor::tokenize_lines_rules` runs it behind `fill_tags` in the same one call.
pub struct PatternMatchTagger<'p> {
    raw: *mut std::ffi::c_void,
    predictor: &'p HipPredictor,
}
// immutable after creation, like the predictor it belongs to
unsafe impl Send for PatternMatchTagger<'_> {}
unsafe impl Sync for PatternMatchTagger<'_> {}

impl<'p> PatternMatchTagger<'p> {
    /// `PatternMatchTagger::new(rules)` (pattern_match_tagger.rs:15-19) for `predictor`; the rules as (surface, tags) pairs -- a `HashMap`'s
    /// `iter()` will do; of a surface given twice the last pair is kept.  Errors name the rule: a surface that is empty or holds a NUL, a tag
    /// that holds a NUL.
    pub fn new<'a, I>(predictor: &'p HipPredictor, rules: I) -> Result<Self>
    where
        I: IntoIterator<Item = (&'a String, &'a Vec<Option<String>>)>,
    {
        let (mut surfaces, mut tags) = (Vec::<u8>::new(), Vec::<u8>::new());
        let (mut offsets, mut tag_offsets) = (vec![0u64], vec![0u64]);
        let (mut slot_counts, mut present) = (Vec::<u32>::new(), Vec::<u8>::new());
        for (surface, list) in rules {
            surfaces.extend_from_slice(surface.as_bytes());
            offsets.push(surfaces.len() as u64);
            slot_counts.push(list.len() as u32);
            for tag in list {
                present.push(tag.is_some() as u8);
                if let Some(t) = tag {
                    tags.extend_from_slice(t.as_bytes());
                }
                tag_offsets.push(tags.len() as u64);
            }
        }
        let n_rules = slot_counts.len();
        // (no dangling pointer of an empty Vec is handed over)
        surfaces.push(0);
        tags.push(0);
        slot_counts.push(0);
        present.push(0);
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            ffi::vpt_pattern_tagger_create(predictor.raw, surfaces.as_ptr(), offsets.as_ptr(), n_rules, slot_counts.as_ptr(), present.as_ptr(), tags.as_ptr(),
                                           tag_offsets.as_ptr(), &mut raw)
        })?;
        Ok(Self { raw, predictor })
    }

    /// The distinct tag strings of the rules: a rule tag is `-(2 + id)`, `id < n_tags()`, wherever the C ABI hands out tag indices.
    pub fn n_tags(&self) -> Result<u32> {
        let mut n = 0u32;
        check(unsafe { ffi::vpt_pattern_tagger_n_tags(self.raw, &mut n) })?;
        Ok(n)
    }

    /// The string of rule tag `id`.
    pub fn tag(&self, id: u32) -> Result<String> {
        let (mut bytes, mut len) = (std::ptr::null::<u8>(), 0usize);
        check(unsafe { ffi::vpt_pattern_tagger_tag(self.raw, id, &mut bytes, &mut len) })?;
        let slice = if len == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(bytes, len) } };
        Ok(String::from_utf8_lossy(slice).into_owned())
    }

    /// The most bytes one rule's tags take in the tokenized text (added to the predictor's bound while the tagger is used).
    pub fn max_tag_suffix(&self) -> Result<u32> {
        let mut n = 0u32;
        check(unsafe { ffi::vpt_pattern_tagger_max_tag_suffix(self.raw, &mut n) })?;
        Ok(n)
    }
}

impl Drop for PatternMatchTagger<'_> {
    fn drop(&mut self) {
        unsafe { ffi::vpt_pattern_tagger_destroy(self.raw) }
    }
}

impl HipPredictor {
    /// `tokenize_lines(.., tagged = true)` with `tagger.filter(&mut sentence)` behind every `fill_tags` (pattern_match_tagger.rs:21-41), in the
    /// same one call: the rule tags are printed with the tag models'.  The tagger must have been made for this predictor.
    pub fn tokenize_lines_rules<'a, I: IntoIterator<Item = &'a str>>(&self, lines: I, flags: u32, tagger: &PatternMatchTagger<'_>) -> Result<Vec<String>> {
        if !std::ptr::eq(tagger.predictor, self) {
            return Err(HipError::InvalidArgument("InvalidArgumentError: tagger: does not belong to this predictor".to_string()));
        }
        let (utf8, boff) = pack(lines.into_iter());
        let n = boff.len() - 1;
        let mut suffix = 0u32;
        check(unsafe { ffi::vpt_predictor_max_tag_suffix(self.raw, &mut suffix) })?;
        let suffix = suffix as usize + tagger.max_tag_suffix()? as usize;
        let cap = 3 * utf8.len() + 64 + utf8.len() * suffix;
        let mut text = vec![0u8; cap];
        let mut toff = vec![0u64; n + 1];
        check(unsafe {
            ffi::vpt_tokenize_batch_rules(self.raw, utf8.as_ptr(), boff.as_ptr(), n, flags, 1, text.as_mut_ptr(), cap as u64, toff.as_mut_ptr(), tagger.raw)
        })?;
        Ok((0..n).map(|i| String::from_utf8_lossy(&text[toff[i] as usize..toff[i + 1] as usize]).into_owned()).collect())
    }
}

/// A stop set for the tagged token stream (`vpt_tag_stop_create`): (slot, tag string) pairs.  A token is dropped when, for some pair, its slot's
/// tag equals the pair's string -- a tag model's or, with `tagger`, a rule's; `None` never matches; a string in neither vocabulary matches
/// nothing.  Immutable; borrows its predictor (and the tagger whose ids it resolved), which outlive it.
pub struct TagStopFilter<'p> {
    raw: *mut std::ffi::c_void,
    predictor: &'p HipPredictor,
}
unsafe impl Send for TagStopFilter<'_> {}
unsafe impl Sync for TagStopFilter<'_> {}

impl<'p> TagStopFilter<'p> {
    /// Errors name the entry: a slot that is not below the predictor's `n_tags`, a tag that holds a NUL; a tagger of another predictor.
    pub fn new<'a, I>(predictor: &'p HipPredictor, pairs: I, tagger: Option<&'p PatternMatchTagger<'p>>) -> Result<Self>
    where
        I: IntoIterator<Item = (u32, &'a str)>,
    {
        if let Some(t) = tagger {
            if !std::ptr::eq(t.predictor, predictor) {
                return Err(HipError::InvalidArgument("InvalidArgumentError: tagger: does not belong to this predictor".to_string()));
            }
        }
        let (mut slots, mut tags, mut tag_offsets) = (Vec::<u32>::new(), Vec::<u8>::new(), vec![0u64]);
        for (slot, tag) in pairs {
            slots.push(slot);
            tags.extend_from_slice(tag.as_bytes());
            tag_offsets.push(tags.len() as u64);
        }
        let n = slots.len();
        // (no dangling pointer of an empty Vec is handed over)
        slots.push(0);
        tags.push(0);
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            ffi::vpt_tag_stop_create(predictor.raw, tagger.map_or(std::ptr::null(), |t| t.raw as *const std::ffi::c_void), slots.as_ptr(), tags.as_ptr(),
                                     tag_offsets.as_ptr(), n, &mut raw)
        })?;
        Ok(Self { raw, predictor })
    }
}

impl Drop for TagStopFilter<'_> {
    fn drop(&mut self) {
        unsafe { ffi::vpt_tag_stop_destroy(self.raw) }
    }
}

/// A vocabulary for the token stream's ids (`vpt_vocab_create`): entry k of `surfaces` gets id k, a token that is no entry `unk_id`.  Tied to
/// ONE predictor (it borrows it); immutable.  An empty surface, a NUL and a repeated surface are errors that name the entry.
pub struct Vocabulary<'p> {
    raw: *mut std::ffi::c_void,
    predictor: &'p HipPredictor,
    pub unk_id: i32,
}
unsafe impl Send for Vocabulary<'_> {}
unsafe impl Sync for Vocabulary<'_> {}

impl<'p> Vocabulary<'p> {
    pub fn new<'a, I>(predictor: &'p HipPredictor, surfaces: I, unk_id: i32) -> Result<Self>
    where
        I: IntoIterator<Item = &'a str>,
    {
        let (mut bytes, mut offsets) = (Vec::<u8>::new(), vec![0u64]);
        for s in surfaces {
            bytes.extend_from_slice(s.as_bytes());
            offsets.push(bytes.len() as u64);
        }
        let n = offsets.len() - 1;
        bytes.push(0);   // (no dangling pointer of an empty Vec is handed over)
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::vpt_vocab_create(predictor.raw, bytes.as_ptr(), offsets.as_ptr(), n, unk_id, &mut raw) })?;
        Ok(Self { raw, predictor, unk_id })
    }

    /// The surface of `id` (`vpt_vocab_surface`).
    pub fn surface(&self, id: u32) -> Result<String> {
        let (mut bytes, mut len) = (std::ptr::null::<u8>(), 0usize);
        check(unsafe { ffi::vpt_vocab_surface(self.raw as *const std::ffi::c_void, id, &mut bytes, &mut len) })?;
        let slice = if len == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(bytes, len) } };
        Ok(String::from_utf8_lossy(slice).into_owned())
    }

    /// (token_offsets [n + 1], ids) of a packed batch of documents through the untagged stream's steps (`vpt_token_stream_ids_batch`):
    /// `normalize` looks the KyteaFullwidthFilter image of a token up, else the caller's bytes.
    pub fn encode_batch(&self, utf8: &[u8], byte_offsets: &[u64], wsconst_flags: u32, normalize: bool) -> Result<(Vec<u64>, Vec<i32>)> {
        let n = byte_offsets.len().saturating_sub(1);
        let cap = utf8.len() + 1;
        let mut offsets = vec![0u64; n + 1];
        let (mut starts, mut ends, mut positions, mut ids) = (vec![0u32; cap], vec![0u32; cap], vec![0u32; cap], vec![0i32; cap]);
        let text = if utf8.is_empty() { &[0u8][..] } else { utf8 };
        check(unsafe {
            ffi::vpt_token_stream_ids_batch(self.predictor.raw, text.as_ptr(), byte_offsets.as_ptr(), n, wsconst_flags, std::ptr::null(), std::ptr::null(),
                                            self.raw as *const std::ffi::c_void, if normalize { 1 } else { 0 }, offsets.as_mut_ptr(), starts.as_mut_ptr(),
                                            ends.as_mut_ptr(), positions.as_mut_ptr(), std::ptr::null_mut(), ids.as_mut_ptr(), cap as u64)
        })?;
        ids.truncate(offsets[n] as usize);
        Ok((offsets, ids))
    }

    /// The number of entries (`vpt_vocab_info`): the `n_terms` of the postings over this vocabulary.
    pub fn len(&self) -> Result<u32> {
        let mut n = 0u32;
        check(unsafe { ffi::vpt_vocab_info(self.raw as *const std::ffi::c_void, &mut n, std::ptr::null_mut(), std::ptr::null_mut()) })?;
        Ok(n)
    }

    /// The postings of a packed batch of documents (a segment) through the untagged stream's steps (`vpt_token_stream_postings_batch`):
    /// term = this vocabulary's id, document = `doc_base` + the document's index (empty documents included), tf = the term's tokens in it.
    /// `byte_offsets` must be non-decreasing and inside `utf8`, `doc_base` + the documents at most 2^32: checked here.
    pub fn index_batch(&self, utf8: &[u8], byte_offsets: &[u64], wsconst_flags: u32, normalize: bool, doc_base: u64) -> Result<Postings> {
        let n = byte_offsets.len().saturating_sub(1);
        if byte_offsets.windows(2).any(|w| w[0] > w[1]) || (n > 0 && byte_offsets[n] > utf8.len() as u64) {
            return Err(HipError::InvalidArgument("InvalidArgumentError: byte_offsets: must be non-decreasing and inside the text".into()));
        }
        if doc_base > 1 << 32 || n as u64 > (1u64 << 32) - doc_base {
            return Err(HipError::InvalidArgument("InvalidArgumentError: doc_base: doc_base + n_documents must not exceed 2^32".into()));
        }
        let cap = utf8.len() + 1;   // (a token has a byte at least, a posting a token)
        let mut term_offsets = vec![0u64; self.len()? as usize + 1];
        let (mut docs, mut tfs) = (vec![0u32; cap], vec![0u32; cap]);
        let (mut n_postings, mut n_dropped) = (0u64, 0u64);
        let text = if utf8.is_empty() { &[0u8][..] } else { utf8 };
        let offsets = if byte_offsets.is_empty() { &[0u64][..] } else { byte_offsets };
        check(unsafe {
            ffi::vpt_token_stream_postings_batch(self.predictor.raw, text.as_ptr(), offsets.as_ptr(), n, wsconst_flags, std::ptr::null(), std::ptr::null(),
                                                 self.raw as *const std::ffi::c_void, if normalize { 1 } else { 0 }, doc_base, term_offsets.as_mut_ptr(),
                                                 docs.as_mut_ptr(), tfs.as_mut_ptr(), cap as u64, &mut n_postings, &mut n_dropped)
        })?;
        docs.truncate(n_postings as usize);
        tfs.truncate(n_postings as usize);
        Ok(Postings { term_offsets, docs, tfs, n_dropped, n_combined: 0 })
    }
}

/// The postings of one batch of documents (a segment), term-major: term k's postings are `term_offsets[k] .. term_offsets[k + 1]` of `docs`
/// (`doc_base` + the document's index, ascending within a term) and `tfs`.  `n_dropped`: the tokens whose id was no term.
#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Postings {
    pub term_offsets: Vec<u64>,
    pub docs: Vec<u32>,
    pub tfs: Vec<u32>,
    pub n_dropped: u64,
    /// After `merge`: the input postings that were combined into another.
    pub n_combined: u64,
}

/// `vpt_postings_segment` of include/vaporetto_hip.h, field by field (host pointers for `vpt_postings_merge`).
#[repr(C)]
struct PostingsSegment {
    term_offsets: *const u64,
    docs: *const u32,
    tfs: *const u32,
    n_terms: u32,
    capacity: u64,
}

/// `vpt_postings_positional_segment` of include/vaporetto_hip.h, field by field (host pointers for `vpt_postings_merge_positional`).
#[repr(C)]
struct PostingsPositionalSegment {
    term_offsets: *const u64,
    docs: *const u32,
    tfs: *const u32,
    first: *const u64,
    positions: *const u32,
    n_terms: u32,
    capacity: u64,
    capacity_positions: u64,
}

impl Postings {
    /// The merge of segments that share a term id space (`vpt_postings_merge`): per term the union of their lists by document, a document
    /// that stands in several of them one posting whose tf is the sum; `n_dropped` the segments' sum.  `ordered`: the promise that every
    /// segment's documents are above those of the one before -- checked on the device, no sort.  `n_terms`: the merged term count, at least
    /// every segment's.  The segments' arrays must belong together: checked here.
    pub fn merge(predictor: &Predictor, segments: &[Postings], ordered: bool, n_terms: u32) -> Result<Postings> {
        let mut segs = Vec::with_capacity(segments.len());
        let mut cap = 0usize;
        for s in segments {
            let n = s.term_offsets.len();
            if n == 0 || n - 1 > n_terms as usize || s.docs.len() != s.tfs.len() || s.term_offsets[n - 1] > s.docs.len() as u64 {
                return Err(HipError::InvalidArgument("InvalidArgumentError: merge: a segment's arrays do not belong together".into()));
            }
            segs.push(PostingsSegment { term_offsets: s.term_offsets.as_ptr(), docs: s.docs.as_ptr(), tfs: s.tfs.as_ptr(), n_terms: (n - 1) as u32,
                                        capacity: s.docs.len() as u64 });
            cap += s.docs.len();
        }
        let mut term_offsets = vec![0u64; n_terms as usize + 1];
        let (mut docs, mut tfs) = (vec![0u32; cap + 1], vec![0u32; cap + 1]);
        let (mut n_postings, mut n_combined) = (0u64, 0u64);
        check(unsafe {
            ffi::vpt_postings_merge(predictor.raw, segs.as_ptr() as *const std::ffi::c_void, segs.len(), n_terms, if ordered { 1 } else { 0 },
                                    term_offsets.as_mut_ptr(), docs.as_mut_ptr(), tfs.as_mut_ptr(), cap as u64, &mut n_postings, &mut n_combined)
        })?;
        docs.truncate(n_postings as usize);
        tfs.truncate(n_postings as usize);
        Ok(Postings { term_offsets, docs, tfs, n_dropped: segments.iter().map(|s| s.n_dropped).sum(), n_combined })
    }

    /// The merge of POSITIONAL segments (`vpt_postings_merge_positional`): `merge`, with the position lists carried along.  A segment is its
    /// postings, its `first` (`docs.len() + 1` entries) and its `positions` (`first[docs.len()]` of them), as
    /// `vpt_token_stream_positional_postings_batch` returns them.  Returns the merged postings with their `first` and `positions`: a merged
    /// posting's list is the ascending union of its inputs' lists (an equal position in two of them is an error), what `phrase_search` takes.
    pub fn merge_positional(predictor: &Predictor, segments: &[(&Postings, &[u64], &[u32])], ordered: bool, n_terms: u32)
                            -> Result<(Postings, Vec<u64>, Vec<u32>)> {
        let mut segs = Vec::with_capacity(segments.len());
        let (mut cap, mut cap_pos) = (0usize, 0usize);
        for (s, first, positions) in segments {
            let n = s.term_offsets.len();
            if n == 0 || n - 1 > n_terms as usize || s.docs.len() != s.tfs.len() || s.term_offsets[n - 1] > s.docs.len() as u64
                || first.len() != s.docs.len() + 1 || first[s.docs.len()] > positions.len() as u64 {
                return Err(HipError::InvalidArgument("InvalidArgumentError: merge: a segment's arrays do not belong together".into()));
            }
            segs.push(PostingsPositionalSegment { term_offsets: s.term_offsets.as_ptr(), docs: s.docs.as_ptr(), tfs: s.tfs.as_ptr(), first: first.as_ptr(),
                                                  positions: positions.as_ptr(), n_terms: (n - 1) as u32, capacity: s.docs.len() as u64,
                                                  capacity_positions: positions.len() as u64 });
            cap += s.docs.len();
            cap_pos += positions.len();
        }
        let mut term_offsets = vec![0u64; n_terms as usize + 1];
        let (mut docs, mut tfs, mut first, mut positions) = (vec![0u32; cap + 1], vec![0u32; cap + 1], vec![0u64; cap + 1], vec![0u32; cap_pos + 1]);
        let (mut n_postings, mut n_combined, mut n_positions) = (0u64, 0u64, 0u64);
        check(unsafe {
            ffi::vpt_postings_merge_positional(predictor.raw, segs.as_ptr() as *const std::ffi::c_void, segs.len(), n_terms, if ordered { 1 } else { 0 },
                                               term_offsets.as_mut_ptr(), docs.as_mut_ptr(), tfs.as_mut_ptr(), first.as_mut_ptr(), cap as u64,
                                               positions.as_mut_ptr(), cap_pos as u64, &mut n_postings, &mut n_combined, &mut n_positions)
        })?;
        docs.truncate(n_postings as usize);
        tfs.truncate(n_postings as usize);
        first.truncate(n_postings as usize + 1);
        positions.truncate(n_positions as usize);
        Ok((Postings { term_offsets, docs, tfs, n_dropped: segments.iter().map(|(s, _, _)| s.n_dropped).sum(), n_combined }, first, positions))
    }

    /// BM25 top-k of every query over this segment (`vpt_postings_search`; the definition is in include/vaporetto_hip.h).  `queries`: term ids, a
    /// slot per id, ids outside the vocabulary score nothing, each weighted with `vpt_okapi_idf(n_documents, df)`.  `doc_lens[i]`: the length of
    /// document `doc_base + i`; avgdl = their mean, computed in f64 and rounded to f32.  Returns per query at most `k` (document, score) pairs by
    /// score descending, then document ascending, and the queries' match counts.
    pub fn search(&self, predictor: &Predictor, queries: &[Vec<i32>], doc_lens: &[u32], doc_base: u64, k: u32, k1: f32, b: f32)
                  -> Result<(Vec<Vec<(u32, f32)>>, Vec<u64>)> {
        if queries.is_empty() {
            return Ok((Vec::new(), Vec::new()));
        }
        let n = self.term_offsets.len();
        if n == 0 || doc_lens.is_empty() || self.docs.len() != self.tfs.len() || self.term_offsets[n - 1] > self.docs.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: search: the arrays do not belong together".into()));
        }
        let avgdl = (doc_lens.iter().map(|&l| l as f64).sum::<f64>() / doc_lens.len() as f64) as f32;
        let mut offsets = vec![0u64];
        let (mut terms, mut weights) = (Vec::new(), Vec::new());
        for q in queries {
            for &t in q {
                let mut w = 0f32;
                if t >= 0 && (t as usize) < n - 1 {
                    check(unsafe { ffi::vpt_okapi_idf(doc_lens.len() as u64, self.df(t as usize), &mut w) })?;
                }
                terms.push(t);
                weights.push(w);
            }
            offsets.push(terms.len() as u64);
        }
        terms.push(0);
        weights.push(0f32);
        let n_out = queries.len() * k as usize + 1;
        let (mut hit_docs, mut hit_scores) = (vec![0u32; n_out], vec![0f32; n_out]);
        let (mut hit_counts, mut match_counts, mut counts) = (vec![0u32; queries.len()], vec![0u64; queries.len()], [0u64; 3]);
        check(unsafe {
            ffi::vpt_postings_search(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(), (n - 1) as u32, doc_base,
                                     doc_lens.len() as u64, doc_lens.as_ptr(), offsets.as_ptr(), terms.as_ptr(), weights.as_ptr(), queries.len() as u32,
                                     k1, b, avgdl, k, hit_docs.as_mut_ptr(), hit_scores.as_mut_ptr(), hit_counts.as_mut_ptr(), match_counts.as_mut_ptr(),
                                     counts.as_mut_ptr())
        })?;
        let hits = (0..queries.len())
            .map(|q| (0..hit_counts[q] as usize).map(|j| (hit_docs[q * k as usize + j], hit_scores[q * k as usize + j])).collect())
            .collect();
        Ok((hits, match_counts))
    }

    /// BM25 top-k of every boolean query over this segment (`vpt_postings_boolean_search`; the definition is in include/vaporetto_hip.h).  A
    /// slot is `(term, occur)`, occur 0 SHOULD, 1 MUST, 2 MUST_NOT: a document matches when every MUST slot has it, no MUST_NOT slot has it
    /// and, without a MUST slot, some SHOULD slot has it.  MUST and SHOULD slots are weighted with `vpt_okapi_idf(n_documents, df)`, MUST_NOT
    /// slots with 0.  `doc_lens`, avgdl and the return value: as in `search`.
    pub fn boolean_search(&self, predictor: &Predictor, queries: &[Vec<(i32, u8)>], doc_lens: &[u32], doc_base: u64, k: u32, k1: f32, b: f32)
                          -> Result<(Vec<Vec<(u32, f32)>>, Vec<u64>)> {
        if queries.is_empty() {
            return Ok((Vec::new(), Vec::new()));
        }
        let n = self.term_offsets.len();
        if n == 0 || doc_lens.is_empty() || self.docs.len() != self.tfs.len() || self.term_offsets[n - 1] > self.docs.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: boolean_search: the arrays do not belong together".into()));
        }
        let avgdl = (doc_lens.iter().map(|&l| l as f64).sum::<f64>() / doc_lens.len() as f64) as f32;
        let mut offsets = vec![0u64];
        let (mut terms, mut weights, mut occurs) = (Vec::new(), Vec::new(), Vec::new());
        for q in queries {
            for &(t, occur) in q {
                let mut w = 0f32;
                if occur != 2 && t >= 0 && (t as usize) < n - 1 {
                    check(unsafe { ffi::vpt_okapi_idf(doc_lens.len() as u64, self.df(t as usize), &mut w) })?;
                }
                terms.push(t);
                weights.push(w);
                occurs.push(occur);
            }
            offsets.push(terms.len() as u64);
        }
        terms.push(0);
        weights.push(0f32);
        occurs.push(0u8);
        let n_out = queries.len() * k as usize + 1;
        let (mut hit_docs, mut hit_scores) = (vec![0u32; n_out], vec![0f32; n_out]);
        let (mut hit_counts, mut match_counts, mut counts) = (vec![0u32; queries.len()], vec![0u64; queries.len()], [0u64; 3]);
        check(unsafe {
            ffi::vpt_postings_boolean_search(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(), (n - 1) as u32, doc_base,
                                             doc_lens.len() as u64, doc_lens.as_ptr(), offsets.as_ptr(), terms.as_ptr(), weights.as_ptr(),
                                             occurs.as_ptr(), queries.len() as u32, k1, b, avgdl, k, hit_docs.as_mut_ptr(), hit_scores.as_mut_ptr(),
                                             hit_counts.as_mut_ptr(), match_counts.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        let hits = (0..queries.len())
            .map(|q| (0..hit_counts[q] as usize).map(|j| (hit_docs[q * k as usize + j], hit_scores[q * k as usize + j])).collect())
            .collect();
        Ok((hits, match_counts))
    }

    /// BM25 top-k of every boolean query of CLAUSES over this segment and its position lists (`vpt_postings_clause_search`; the definition is in
    /// include/vaporetto_hip.h).  `first` and `positions`: as in `phrase_search`.  A clause is `(terms, occur)`, occur 0 SHOULD, 1 MUST, 2
    /// MUST_NOT: a clause of one term is a slot of that term, as in `boolean_search`; every other clause is ONE exact phrase scored by its
    /// phrase frequency (an id outside the vocabulary makes it match nothing, and so does an empty clause).  The weight of a MUST or SHOULD
    /// clause is the phrase weight of `phrase_search` (the f32 sum in slot order of `vpt_okapi_idf` over its terms), of a MUST_NOT clause 0.
    /// `doc_lens`, avgdl and the return value: as in `search`.
    pub fn clause_search(&self, predictor: &Predictor, first: &[u64], positions: &[u32], queries: &[Vec<(Vec<i32>, u8)>], doc_lens: &[u32],
                         doc_base: u64, k: u32, k1: f32, b: f32)
                         -> Result<(Vec<Vec<(u32, f32)>>, Vec<u64>)> {
        if queries.is_empty() {
            return Ok((Vec::new(), Vec::new()));
        }
        let n = self.term_offsets.len();
        if n == 0 || doc_lens.is_empty() || self.docs.len() != self.tfs.len() || self.term_offsets[n - 1] != self.docs.len() as u64
            || first.len() != self.docs.len() + 1 || first[first.len() - 1] != positions.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: clause_search: the arrays do not belong together".into()));
        }
        let avgdl = (doc_lens.iter().map(|&l| l as f64).sum::<f64>() / doc_lens.len() as f64) as f32;
        let (mut offsets, mut clause_offsets) = (vec![0u64], vec![0u64]);
        let (mut terms, mut weights, mut occurs) = (Vec::new(), Vec::new(), Vec::new());
        for q in queries {
            for (clause, occur) in q {
                let mut sum: Option<f32> = None;
                for &t in clause {
                    terms.push(t);
                    if *occur == 2 || t < 0 || (t as usize) >= n - 1 {
                        continue;
                    }
                    let mut w = 0f32;
                    check(unsafe { ffi::vpt_okapi_idf(doc_lens.len() as u64, self.df(t as usize), &mut w) })?;
                    sum = Some(match sum { Some(s) => s + w, None => w });
                }
                weights.push(sum.unwrap_or(0f32));
                occurs.push(*occur);
                clause_offsets.push(terms.len() as u64);
            }
            offsets.push(occurs.len() as u64);
        }
        terms.push(0);
        weights.push(0f32);
        occurs.push(0u8);
        let mut pos = positions.to_vec();
        pos.push(0);
        let n_out = queries.len() * k as usize + 1;
        let (mut hit_docs, mut hit_scores) = (vec![0u32; n_out], vec![0f32; n_out]);
        let (mut hit_counts, mut match_counts, mut counts) = (vec![0u32; queries.len()], vec![0u64; queries.len()], [0u64; 3]);
        check(unsafe {
            ffi::vpt_postings_clause_search(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(), first.as_ptr(),
                                            pos.as_ptr(), (n - 1) as u32, doc_base, doc_lens.len() as u64, doc_lens.as_ptr(), offsets.as_ptr(),
                                            clause_offsets.as_ptr(), terms.as_ptr(), weights.as_ptr(), occurs.as_ptr(), queries.len() as u32, k1, b,
                                            avgdl, k, hit_docs.as_mut_ptr(), hit_scores.as_mut_ptr(), hit_counts.as_mut_ptr(),
                                            match_counts.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        let hits = (0..queries.len())
            .map(|q| (0..hit_counts[q] as usize).map(|j| (hit_docs[q * k as usize + j], hit_scores[q * k as usize + j])).collect())
            .collect();
        Ok((hits, match_counts))
    }

    /// Exact-phrase BM25 top-k of every phrase over this segment and its position lists (`vpt_postings_phrase_search`; the definition is in
    /// include/vaporetto_hip.h).  `first` [postings + 1] and `positions` [indexed tokens]: posting q's positions are
    /// `positions[first[q] .. first[q + 1]]`, strictly ascending (what `vpt_token_stream_positional_postings_batch` returns).  `phrases`: term
    /// ids, each ONE phrase, its ids at consecutive positions in order; an id outside the vocabulary makes it match nothing.  The weight of a
    /// phrase is tantivy's: the f32 sum, in slot order, of `vpt_okapi_idf` over its slots.  Returns per phrase at most `k`
    /// (document, score, frequency) by score descending, then document ascending, and the match counts.
    pub fn phrase_search(&self, predictor: &Predictor, first: &[u64], positions: &[u32], phrases: &[Vec<i32>], doc_lens: &[u32], doc_base: u64,
                         k: u32, k1: f32, b: f32) -> Result<(Vec<Vec<(u32, f32, u32)>>, Vec<u64>)> {
        self.phrase_search_with(predictor, first, positions, phrases, None, doc_lens, doc_base, k, k1, b)
    }

    /// `phrase_search` with a slop budget per phrase (`vpt_postings_sloppy_phrase_search`; tantivy's `PhraseQuery::set_slop`, the definition
    /// is in include/vaporetto_hip.h): `slops[q]` in 0 ..= 31 is phrase q's; the frequency of a hit is the number of distinct occurrences
    /// under that slop.  With every slop 0 the result is `phrase_search`'s.
    pub fn sloppy_phrase_search(&self, predictor: &Predictor, first: &[u64], positions: &[u32], phrases: &[Vec<i32>], slops: &[u32],
                                doc_lens: &[u32], doc_base: u64, k: u32, k1: f32, b: f32)
                                -> Result<(Vec<Vec<(u32, f32, u32)>>, Vec<u64>)> {
        if slops.len() != phrases.len() {
            return Err(HipError::InvalidArgument("InvalidArgumentError: slops: one per phrase".into()));
        }
        self.phrase_search_with(predictor, first, positions, phrases, Some(slops), doc_lens, doc_base, k, k1, b)
    }

    /// The posting list of every phrase under its slop (`vpt_postings_sloppy_phrase_lists`): `(list_offsets, list_docs, list_tfs)`, list q the
    /// entries `list_offsets[q] .. list_offsets[q + 1]`: the global numbers of the documents that match phrase q, ascending, and their
    /// phrase frequencies -- what `vpt_postings_clause_search_device` takes as derived lists.
    pub fn sloppy_phrase_lists(&self, predictor: &Predictor, first: &[u64], positions: &[u32], phrases: &[Vec<i32>], slops: &[u32],
                               n_documents: u64, doc_base: u64) -> Result<(Vec<u64>, Vec<u32>, Vec<u32>)> {
        if phrases.is_empty() {
            return Ok((vec![0u64], Vec::new(), Vec::new()));
        }
        let n = self.term_offsets.len();
        if n == 0 || slops.len() != phrases.len() || self.docs.len() != self.tfs.len() || self.term_offsets[n - 1] != self.docs.len() as u64
            || first.len() != self.docs.len() + 1 || first[first.len() - 1] != positions.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: sloppy_phrase_lists: the arrays do not belong together".into()));
        }
        let mut offsets = vec![0u64];
        let mut terms = Vec::new();
        let mut capacity = 0u64;   // per phrase the smallest df among its terms: what always suffices
        for q in phrases {
            let mut bound: Option<u64> = None;
            for &t in q {
                let df = if t >= 0 && (t as usize) < n - 1 { self.df(t as usize) } else { 0 };
                bound = Some(match bound { Some(x) => x.min(df), None => df });
                terms.push(t);
            }
            capacity += bound.unwrap_or(0);
            offsets.push(terms.len() as u64);
        }
        terms.push(0);
        let mut pos = positions.to_vec();
        pos.push(0);
        let mut list_offsets = vec![0u64; phrases.len() + 1];
        let (mut list_docs, mut list_tfs) = (vec![0u32; capacity as usize + 1], vec![0u32; capacity as usize + 1]);
        let mut counts = [0u64; 3];
        check(unsafe {
            ffi::vpt_postings_sloppy_phrase_lists(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(), first.as_ptr(),
                                                  pos.as_ptr(), (n - 1) as u32, doc_base, n_documents, offsets.as_ptr(), terms.as_ptr(),
                                                  slops.as_ptr(), phrases.len() as u32, list_offsets.as_mut_ptr(), list_docs.as_mut_ptr(),
                                                  list_tfs.as_mut_ptr(), capacity, counts.as_mut_ptr())
        })?;
        list_docs.truncate(counts[1] as usize);
        list_tfs.truncate(counts[1] as usize);
        Ok((list_offsets, list_docs, list_tfs))
    }

    fn phrase_search_with(&self, predictor: &Predictor, first: &[u64], positions: &[u32], phrases: &[Vec<i32>], slops: Option<&[u32]>,
                          doc_lens: &[u32], doc_base: u64, k: u32, k1: f32, b: f32) -> Result<(Vec<Vec<(u32, f32, u32)>>, Vec<u64>)> {
        if phrases.is_empty() {
            return Ok((Vec::new(), Vec::new()));
        }
        let n = self.term_offsets.len();
        if n == 0 || doc_lens.is_empty() || self.docs.len() != self.tfs.len() || self.term_offsets[n - 1] != self.docs.len() as u64
            || first.len() != self.docs.len() + 1 || first[first.len() - 1] != positions.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: phrase_search: the arrays do not belong together".into()));
        }
        let avgdl = (doc_lens.iter().map(|&l| l as f64).sum::<f64>() / doc_lens.len() as f64) as f32;
        let mut offsets = vec![0u64];
        let (mut terms, mut weights) = (Vec::new(), Vec::new());
        for q in phrases {
            let mut sum: Option<f32> = None;
            for &t in q {
                if t >= 0 && (t as usize) < n - 1 {
                    let mut w = 0f32;
                    check(unsafe { ffi::vpt_okapi_idf(doc_lens.len() as u64, self.df(t as usize), &mut w) })?;
                    sum = Some(match sum { Some(s) => s + w, None => w });
                }
                terms.push(t);
            }
            weights.push(sum.unwrap_or(0f32));
            offsets.push(terms.len() as u64);
        }
        terms.push(0);
        let mut pos = positions.to_vec();
        pos.push(0);
        let n_out = phrases.len() * k as usize + 1;
        let (mut hit_docs, mut hit_scores, mut hit_freqs) = (vec![0u32; n_out], vec![0f32; n_out], vec![0u32; n_out]);
        let (mut hit_counts, mut match_counts, mut counts) = (vec![0u32; phrases.len()], vec![0u64; phrases.len()], [0u64; 3]);
        check(unsafe {
            match slops {
                None => ffi::vpt_postings_phrase_search(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(),
                                                        first.as_ptr(), pos.as_ptr(), (n - 1) as u32, doc_base, doc_lens.len() as u64,
                                                        doc_lens.as_ptr(), offsets.as_ptr(), terms.as_ptr(), weights.as_ptr(), phrases.len() as u32,
                                                        k1, b, avgdl, k, hit_docs.as_mut_ptr(), hit_scores.as_mut_ptr(), hit_freqs.as_mut_ptr(),
                                                        hit_counts.as_mut_ptr(), match_counts.as_mut_ptr(), counts.as_mut_ptr()),
                Some(s) => ffi::vpt_postings_sloppy_phrase_search(predictor.raw, self.term_offsets.as_ptr(), self.docs.as_ptr(), self.tfs.as_ptr(),
                                                                  first.as_ptr(), pos.as_ptr(), (n - 1) as u32, doc_base, doc_lens.len() as u64,
                                                                  doc_lens.as_ptr(), offsets.as_ptr(), terms.as_ptr(), weights.as_ptr(), s.as_ptr(),
                                                                  phrases.len() as u32, k1, b, avgdl, k, hit_docs.as_mut_ptr(),
                                                                  hit_scores.as_mut_ptr(), hit_freqs.as_mut_ptr(), hit_counts.as_mut_ptr(),
                                                                  match_counts.as_mut_ptr(), counts.as_mut_ptr()),
            }
        })?;
        let hits = (0..phrases.len())
            .map(|q| (0..hit_counts[q] as usize).map(|j| { let at = q * k as usize + j; (hit_docs[at], hit_scores[at], hit_freqs[at]) }).collect())
            .collect();
        Ok((hits, match_counts))
    }

    /// The document frequency of `term`.
    pub fn df(&self, term: usize) -> u64 {
        self.term_offsets[term + 1] - self.term_offsets[term]
    }

    /// (docs, tfs) of `term`.
    pub fn postings(&self, term: usize) -> (&[u32], &[u32]) {
        let (a, b) = (self.term_offsets[term] as usize, self.term_offsets[term + 1] as usize);
        (&self.docs[a..b], &self.tfs[a..b])
    }
}

impl Drop for Vocabulary<'_> {
    fn drop(&mut self) {
        unsafe { ffi::vpt_vocab_destroy(self.raw) }
    }
}

/// A vocabulary counter (`vpt_vocab_counter_create`): token surface -> count, accumulated on the predictor's device; `finish` is what
/// `Vocabulary::new` takes.  Tied to ONE predictor (it borrows it).  The handle is mutable and takes one call at a time: the methods that
/// count take `&mut self`, and the type is `Send` but not `Sync`.
pub struct VocabularyCounter<'p> {
    raw: *mut std::ffi::c_void,
    predictor: &'p HipPredictor,
}
unsafe impl Send for VocabularyCounter<'_> {}

/// `vpt_vocab_counter_info`.
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct VocabularyCounterInfo {
    pub n_keys: u64,
    pub n_counted: u64,
    pub n_skipped: u64,
    pub n_slots: u32,
    pub full: bool,
}

impl<'p> VocabularyCounter<'p> {
    /// `max_keys`: 1 ..= 2^24 distinct surfaces; `max_surface_chars`: 1 ..= 2^24, a longer token is skipped; `arena_chars`: the code points
    /// kept over all keys, 0 = 8 * max_keys, below 2^32.  Checked here before anything is handed to C.
    pub fn new(predictor: &'p HipPredictor, max_keys: u64, max_surface_chars: u64, arena_chars: u64) -> Result<Self> {
        if max_keys < 1 || max_keys > 1 << 24 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: max_keys: must be between 1 and 2^24".into()));
        }
        if max_surface_chars < 1 || max_surface_chars > 1 << 24 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: max_surface_chars: must be between 1 and 2^24".into()));
        }
        if arena_chars > 0xFFFF_FFF0 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: arena_chars: must be below 2^32".into()));
        }
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::vpt_vocab_counter_create(predictor.raw, max_keys, max_surface_chars, arena_chars, &mut raw) })?;
        Ok(Self { raw, predictor })
    }

    pub fn reset(&mut self) -> Result<()> {
        check(unsafe { ffi::vpt_vocab_counter_reset(self.raw) })
    }

    pub fn info(&mut self) -> Result<VocabularyCounterInfo> {
        let (mut k, mut c, mut s, mut n, mut f) = (0u64, 0u64, 0u64, 0u32, 0u32);
        check(unsafe { ffi::vpt_vocab_counter_info(self.raw, &mut k, &mut c, &mut s, &mut n, &mut f) })?;
        Ok(VocabularyCounterInfo { n_keys: k, n_counted: c, n_skipped: s, n_slots: n, full: f != 0 })
    }

    /// Every token of a packed batch of documents through the untagged stream's steps into the counter (`vpt_token_stream_count_batch`);
    /// `normalize` counts the KyteaFullwidthFilter image of a token, else the caller's bytes.  `byte_offsets` must be non-decreasing, start
    /// inside `utf8` and end at most at its length: checked here.
    pub fn count_batch(&mut self, utf8: &[u8], byte_offsets: &[u64], wsconst_flags: u32, normalize: bool) -> Result<()> {
        let n = byte_offsets.len().saturating_sub(1);
        if n == 0 {
            return Ok(());
        }
        if byte_offsets.windows(2).any(|w| w[0] > w[1]) || byte_offsets[n] > utf8.len() as u64 {
            return Err(HipError::InvalidArgument("InvalidArgumentError: byte_offsets: must be non-decreasing and inside the text".into()));
        }
        let text = if utf8.is_empty() { &[0u8][..] } else { utf8 };
        check(unsafe {
            ffi::vpt_token_stream_count_batch(self.predictor.raw, text.as_ptr(), byte_offsets.as_ptr(), n, wsconst_flags, std::ptr::null(),
                                              std::ptr::null(), self.raw, if normalize { 1 } else { 0 })
        })
    }

    /// A snapshot (`vpt_vocab_counter_finish`): (surface, count) of the keys of count >= `min_count`, by count descending, then by code
    /// points ascending; the first `max_entries` of them (0: all).
    pub fn finish(&mut self, min_count: u64, max_entries: u64) -> Result<Vec<(String, u64)>> {
        let (mut s, mut off, mut cnt, mut n) = (std::ptr::null::<u8>(), std::ptr::null::<u64>(), std::ptr::null::<u64>(), 0usize);
        check(unsafe { ffi::vpt_vocab_counter_finish(self.raw, min_count, max_entries, &mut s, &mut off, &mut cnt, &mut n) })?;
        let mut out = Vec::with_capacity(n);
        if n == 0 {
            return Ok(out);
        }
        let (off, cnt) = unsafe { (std::slice::from_raw_parts(off, n + 1), std::slice::from_raw_parts(cnt, n)) };
        let bytes = unsafe { std::slice::from_raw_parts(s, off[n] as usize) };
        for k in 0..n {
            out.push((String::from_utf8_lossy(&bytes[off[k] as usize..off[k + 1] as usize]).into_owned(), cnt[k]));
        }
        Ok(out)
    }
}

impl Drop for VocabularyCounter<'_> {
    fn drop(&mut self) {
        unsafe { ffi::vpt_vocab_counter_destroy(self.raw) }
    }
}

/// What `HipPredictor::token_stream_tagged_batch` returns, over the KEPT tokens: document i owns entries `offsets[i] .. offsets[i + 1]`;
/// `starts` / `ends` are a token's `offset_from` / `offset_to` from its document's first byte, `positions` its index in the document BEFORE
/// filtering, `tags[token * n_tags + slot]` an id of `tag_strings()` (>= 0), -1 (`None`) or -(2 + id) (a rule tag of the tagger).
pub struct TaggedTokens {
    pub offsets: Vec<u64>,
    pub starts: Vec<u32>,
    pub ends: Vec<u32>,
    pub positions: Vec<u32>,
    pub tags: Vec<i32>,
    pub n_tags: usize,
}

impl HipPredictor {
    /// The predictor's tag vocabulary (`vpt_predictor_n_tag_strings` / `vpt_predictor_tag_string`): the distinct raw tag strings of its tag
    /// models in order of first appearance over tag models, slots, candidates.  Empty without `predict_tags`.
    pub fn tag_strings(&self) -> Result<Vec<String>> {
        let mut n = 0u32;
        check(unsafe { ffi::vpt_predictor_n_tag_strings(self.raw, &mut n) })?;
        let mut out = Vec::with_capacity(n as usize);
        for id in 0..n {
            let (mut bytes, mut len) = (std::ptr::null::<u8>(), 0usize);
            check(unsafe { ffi::vpt_predictor_tag_string(self.raw, id, &mut bytes, &mut len) })?;
            let slice = if len == 0 { &[][..] } else { unsafe { std::slice::from_raw_parts(bytes, len) } };
            out.push(String::from_utf8_lossy(slice).into_owned());
        }
        Ok(out)
    }

    /// `token_stream_batch` with every token's tags and, with `stop`, without the stopped tokens (`vpt_token_stream_tagged_batch`): one call,
    /// everything behind the copy in on the device.  The predictor must have been made with `predict_tags`; `tagger` and `stop` for it.  The C
    /// side trusts the sizes, so they are checked here.
    pub fn token_stream_tagged_batch(&self, utf8: &[u8], boff: &[u64], wsconst_flags: u32, tagger: Option<&PatternMatchTagger<'_>>,
                                     stop: Option<&TagStopFilter<'_>>) -> Result<TaggedTokens> {
        let bad = |what: &str| Err(HipError::InvalidArgument(format!("InvalidArgumentError: {}", what)));
        if boff.is_empty() { return bad("byte_offsets: n + 1 entries"); }
        let n = boff.len() - 1;
        if boff.windows(2).any(|w| w[1] < w[0]) { return bad("offsets: must not decrease"); }
        if (utf8.len() as u64) < boff[n] { return bad("utf8: shorter than byte_offsets[n]"); }
        if tagger.map_or(false, |t| !std::ptr::eq(t.predictor, self)) { return bad("tagger: does not belong to this predictor"); }
        if stop.map_or(false, |s| !std::ptr::eq(s.predictor, self)) { return bad("stop: does not belong to this predictor"); }
        let mut nt = 0u32;
        check(unsafe { ffi::vpt_predictor_n_tags(self.raw, &mut nt) })?;
        let n_tags = nt as usize;
        let capacity = ((boff[n] - boff[0]) as usize).max(1);   // a token per char at most, a char per byte at most
        let mut offsets = vec![0u64; n + 1];
        let (mut starts, mut ends, mut positions) = (vec![0u32; capacity], vec![0u32; capacity], vec![0u32; capacity]);
        let mut tags = vec![0i32; capacity * n_tags.max(1)];
        check(unsafe {
            ffi::vpt_token_stream_tagged_batch(self.raw, utf8.as_ptr(), boff.as_ptr(), n, wsconst_flags,
                                               tagger.map_or(std::ptr::null(), |t| t.raw as *const std::ffi::c_void),
                                               stop.map_or(std::ptr::null(), |s| s.raw as *const std::ffi::c_void), offsets.as_mut_ptr(),
                                               starts.as_mut_ptr(), ends.as_mut_ptr(), positions.as_mut_ptr(), tags.as_mut_ptr(), capacity as u64)
        })?;
        let kept = offsets[n] as usize;
        starts.truncate(kept);
        ends.truncate(kept);
        positions.truncate(kept);
        tags.truncate(kept * n_tags);
        Ok(TaggedTokens { offsets, starts, ends, positions, tags, n_tags })
    }
}

/// One batch over the GPUs of a node: `preds[r]` scores the r-th character-balanced range of the sentences (no data-path collective).
/// `boff` / `ooff`: the n + 1 byte / boundary offsets of the n sentences (`vpt_count_boundaries` makes the latter); `scores` and `labels` take
/// `ooff[n]` entries.  The C side trusts these sizes, so they are checked here: a safe function must not let a short slice become a write past it.
pub fn predict_batch_sharded(preds: &[&HipPredictor], utf8: &[u8], boff: &[u64], ooff: &[u64], scores: &mut [i32], labels: &mut [u8], flags: u32) -> Result<()> {
    let bad = |what: &str| Err(HipError::InvalidArgument(format!("InvalidArgumentError: {}", what)));
    if preds.is_empty() { return bad("preds: at least one predictor"); }
    if boff.is_empty() || ooff.len() != boff.len() { return bad("byte_offsets / out_offsets: n + 1 entries each"); }
    let n = boff.len() - 1;
    if boff.windows(2).any(|w| w[1] < w[0]) || ooff.windows(2).any(|w| w[1] < w[0]) { return bad("offsets: must not decrease"); }
    if (utf8.len() as u64) < boff[n] { return bad("utf8: shorter than byte_offsets[n]"); }
    if (scores.len() as u64) < ooff[n] || (labels.len() as u64) < ooff[n] { return bad("scores / labels: shorter than out_offsets[n]"); }
    let raws: Vec<*const ffi::vpt_predictor> = preds.iter().map(|p| p.raw as *const _).collect();
    check(unsafe {
        ffi::vpt_predict_batch_sharded(raws.as_ptr(), raws.len(), utf8.as_ptr(), boff.as_ptr(), n, scores.as_mut_ptr(), labels.as_mut_ptr(), ooff.as_ptr(), flags)
    })
}

fn pack<'a, I: Iterator<Item = &'a str>>(texts: I) -> (Vec<u8>, Vec<u64>) {
    let mut utf8 = Vec::new();
    let mut boff = vec![0u64];
    for t in texts {
        utf8.extend_from_slice(t.as_bytes());
        boff.push(utf8.len() as u64);
    }
    (utf8, boff)
}
