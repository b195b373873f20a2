// CDNA4 YouTube video -> Post JSONL encoder (BASELINE config #4).
//
// MI355X-native equivalent of the reference's convertVideoToPost
// (crawler/youtube/youtube_crawler.go:530-836): engagement formula,
// thumbnail preference, ISO-duration-null handling, OCR rows, performance
// scores, description URL extraction with trailing-punctuation trim +
// dedup (youtube_crawler.go:489-510), sanitized media filename, and the
// same Go-JSON encoding rules. One wave per video, grid-stride; two
// passes share the templated emitter (oracle:
// crawler_amd/youtube/batch.py encode_yt_batch).

#include "common.h"
#include "views.h"

namespace crawl {

struct YtView {
  YtView_FIELDS_0(VIEW_MEMBER)
  int label_len;
  YtView_FIELDS_1(VIEW_MEMBER)
  int created_len;
  YtView_FIELDS_2(VIEW_MEMBER)
  int capture_len;
  int n;
};

// A URL ends at the reference's byte-level whitespace (Go RE2 \S in
// urlPattern, youtube_crawler.go:61: [\t\n\f\r ]) plus this project's
// deliberate < > ". \v, the other control bytes, 0x7F and every
// non-ASCII byte continue a URL. Oracle: convert._URL_RE.
DEV bool url_stop_char(unsigned char c) {
  // one bit per stop byte (all below 64): this test runs once per URL byte
  const unsigned long long stops =
      (1ULL << ' ') | (1ULL << '\t') | (1ULL << '\n') | (1ULL << '\f') |
      (1ULL << '\r') | (1ULL << '<') | (1ULL << '>') | (1ULL << '"');
  return c < 64 && ((stops >> c) & 1ULL);
}
DEV bool url_trim_char(unsigned char c) {
  return c == ',' || c == '.' || c == ';' || c == ':' || c == '!' ||
         c == '?' || c == '(' || c == ')' || c == '\'' || c == '"';
}

// Iterator over the http(s) URL matches of text s[0..n), in order, with
// trailing punctuation trimmed (oracle: convert.extract_urls before its
// dedup). A match is "http://" or "https://" plus AT LEAST ONE non-stop
// byte, and runs to the next stop byte; it yields (start, len) into the
// text itself. Nothing is stored per URL, so any number of URLs costs no
// registers or scratch. Never reads at or past s[n].
struct UrlScan {
  const unsigned char* s;
  int n;
  int p;      // scan position
  int start;  // last match
  int len;
  int last;   // its final byte, s[start + len - 1]

  DEV bool next() {
    while (p + 8 <= n) {  // shortest match: "http://x"
      bool http = s[p] == 'h' && s[p + 1] == 't' && s[p + 2] == 't' &&
                  s[p + 3] == 'p';
      if (!http) { ++p; continue; }
      int q = p + 4;
      if (s[q] == 's') ++q;
      if (!(q + 3 < n && s[q] == ':' && s[q + 1] == '/' &&
            s[q + 2] == '/' && !url_stop_char(s[q + 3]))) {
        ++p;
        continue;
      }
      int end = q + 4;
      while (end < n && !url_stop_char(s[end])) ++end;
      int e2 = end;  // '/' is no trim byte: e2 stays past the "//"
      unsigned char c = s[e2 - 1];
      while (url_trim_char(c)) c = s[--e2 - 1];
      start = p;
      len = e2 - p;
      last = c;
      p = end;
      return true;
    }
    return false;
  }
};

// True when the URL (start, len) already occurred as a match that
// begins in [from, start). Dedup re-scans instead of remembering URLs:
// quadratic in the URL count of one description, which the API caps at
// 5000 bytes. The caller skips the re-scan for a URL whose url_key() no
// earlier URL had.
DEV bool url_seen_before(const unsigned char* s, int n, int from,
                         int start, int len) {
  UrlScan r{s, n, from, 0, 0, 0};
  while (r.next() && r.start < start) {
    if (r.len != len) continue;
    int j = 0;
    while (j < len && s[r.start + j] == s[start + j]) ++j;
    if (j == len) return true;
  }
  return false;
}

// One of 64 filter bits from a URL's length and final byte, both known
// when the scan returns it. Equal URLs have equal keys, so a URL whose
// bit no earlier URL of the description set is new without a re-scan
// (the usual case: a few URLs of different lengths).
DEV unsigned long long url_key(const UrlScan& u) {
  return 1ULL << ((u.len + 5 * u.last) & 63);
}

// YEmit extends the shared JsonEmit (common.h) with the sanitized
// filename writer (runs of non-[A-Za-z0-9._-] -> '_', cap 80;
// convert.sanitize_filename).

template <bool W>
struct YEmit : JsonEmit<W> {
  DEV void rfc(long secs) { this->rfc3339(secs); }
  DEV void sanitized(const unsigned char* s, int n) {
    int o = 0;
    int p = 0;
    while (p < n && o < 80) {
      unsigned char c = s[p];
      bool ok = is_word_char(c) || c == '.' || c == '-';
      if (ok) {
        if (W && lane_id() == 0) this->out[this->cur + o] = c;
        ++o;
        ++p;
      } else {
        if (W && lane_id() == 0) this->out[this->cur + o] = '_';
        ++o;
        while (p < n) {
          unsigned char d = s[p];
          if (is_word_char(d) || d == '.' || d == '-') break;
          ++p;
        }
      }
    }
    this->cur += o;
  }
};

template <bool W>
DEV int emit_yt(const YtView& B, int i, unsigned char* out) {
  YEmit<W> e{};
  e.out = out;
  e.cur = 0;
  const int c = B.channel_idx[i];
  const unsigned char* vid = B.pool + B.vid_off[i];
  const unsigned char* cid = B.pool + B.ch_id_off[c];
  const unsigned char* title = B.pool + B.title_off[i];
  const int title_n = B.title_len[i];
  const unsigned char* desc = B.pool + B.desc_off[i];
  const int desc_n = B.desc_len[i];
  const unsigned char* ctitle = B.pool + B.ch_title_off[c];
  const int ctitle_n = B.ch_title_len[c];
  const long views = B.views[i];
  const int likes = B.likes[i];
  const int comments = B.comments[i];
  const long long engagement =
      (long long)likes + comments + views / 100;

  auto video_url = [&]() {
    LIT(e, "https://www.youtube.com/watch?v=");
    e.raw(vid, 11);
  };
  auto channel_url = [&]() {
    LIT(e, "https://www.youtube.com/channel/");
    e.raw(cid, 24);
  };

  LIT(e, "{\"post_link\":\"");
  video_url();
  LIT(e, "\",\"channel_id\":\"");
  e.raw(cid, 24);
  LIT(e, "\",\"post_uid\":\"");
  e.raw(vid, 11);
  LIT(e, "\",\"url\":\"");
  video_url();
  LIT(e, "\",\"published_at\":\"");
  e.rfc(B.published[i]);
  LIT(e, "\",\"created_at\":\"");
  e.raw(B.created_str, B.created_len);
  LIT(e, "\",\"language_code\":\"");
  e.raw(B.lang_pool + B.lang[i] * 2, 2);
  LIT(e, "\",\"engagement\":");
  e.i64(engagement);
  LIT(e, ",\"view_count\":");
  e.i64(views);
  LIT(e, ",\"like_count\":");
  e.i64(likes);
  LIT(e, ",\"share_count\":0,\"comment_count\":");
  e.i64(comments);
  LIT(e, ",\"crawl_label\":\"");
  e.esc(B.label, B.label_len);
  LIT(e, "\",\"list_ids\":null,\"channel_name\":\"");
  e.esc(ctitle, ctitle_n);
  LIT(e, "\",\"search_terms\":null,\"search_term_ids\":null,"
         "\"project_ids\":null,\"exercise_ids\":null,\"label_data\":null,"
         "\"labels_metadata\":null,\"project_labeled_post_ids\":null,"
         "\"labeler_ids\":null,\"all_labels\":null,\"label_ids\":null,"
         "\"is_ad\":false,\"transcript_text\":\"\",\"image_text\":\"\","
         "\"video_length\":");
  if (B.duration_s[i] < 0) LIT(e, "null");
  else e.i64(B.duration_s[i]);
  LIT(e, ",\"is_verified\":null,\"channel_data\":{\"channel_id\":\"");
  e.raw(cid, 24);
  LIT(e, "\",\"channel_name\":\"");
  e.esc(ctitle, ctitle_n);
  LIT(e, "\",\"channel_description\":\"");
  e.esc(B.pool + B.ch_desc_off[c], B.ch_desc_len[c]);
  LIT(e, "\",\"channel_profile_image\":\"https://i.ytimg.com/ch/");
  e.raw(cid, 24);
  LIT(e, "/default.jpg\",\"channel_engagement_data\":{\"follower_count\":");
  e.i64(B.ch_subs[c]);
  LIT(e, ",\"following_count\":0,\"like_count\":0,\"post_count\":");
  e.i64(B.ch_videos[c]);
  LIT(e, ",\"views_count\":");
  e.i64(B.ch_views[c]);
  LIT(e, ",\"comment_count\":0,\"share_count\":0},"
         "\"channel_url_external\":\"");
  channel_url();
  LIT(e, "\",\"channel_url\":\"");
  channel_url();
  LIT(e, "\",\"country_code\":\"");
  e.esc(B.pool + B.ch_country_off[c], B.ch_country_len[c]);
  LIT(e, "\",\"published_at\":\"");
  e.rfc(B.ch_published[c]);
  LIT(e, "\"},\"platform_name\":\"youtube\",\"shared_id\":null,"
         "\"quoted_id\":null,\"replied_id\":null,\"ai_label\":null,"
         "\"root_post_id\":null,\"engagement_steps_count\":0,"
         "\"ocr_data\":[{\"ocr_text\":\"YouTube thumbnail: default "
         "quality\",\"thumb_url\":\"https://i.ytimg.com/vi/");
  e.raw(vid, 11);
  LIT(e, "/default.jpg\"},{\"ocr_text\":\"YouTube thumbnail: high "
         "quality\",\"thumb_url\":\"https://i.ytimg.com/vi/");
  e.raw(vid, 11);
  LIT(e, "/hq.jpg\"}],\"performance_scores\":{\"likes\":");
  e.i64(likes);
  LIT(e, ",\"shares\":null,\"comments\":");
  e.i64(comments);
  // a float64 in the reference and the oracle: views is valid in
  // 0 .. 2^53 (YouTubeBatch), where the integer prints the same
  LIT(e, ",\"views\":");
  e.i64(views);
  LIT(e, "},\"has_embed_media\":true,\"description\":\"");
  e.esc(desc, desc_n);
  LIT(e, "\",\"repost_channel_data\":null,\"post_type\":[\"video\"],"
         "\"inner_link\":{},\"post_title\":\"");
  e.esc(title, title_n);
  LIT(e, "\",\"media_data\":{\"document_name\":\"");
  e.raw(vid, 11);
  LIT(e, "-");
  e.sanitized(title, title_n);
  LIT(e, ".mp4\"},\"is_reply\":null,\"ad_fields\":null,\"likes_count\":");
  e.i64(likes);
  LIT(e, ",\"shares_count\":0,\"comments_count\":");
  e.i64(comments);
  LIT(e, ",\"views_count\":");
  e.i64(views);
  LIT(e, ",\"searchable_text\":\"");
  e.esc(title, title_n);
  LIT(e, " ");
  e.esc(desc, desc_n);
  LIT(e, "\",\"all_text\":\"");
  e.esc(title, title_n);
  LIT(e, " ");
  e.esc(desc, desc_n);
  LIT(e, "\",\"contrast_agent_project_ids\":null,\"agent_ids\":null,"
         "\"segment_ids\":null,\"thumb_url\":\"https://i.ytimg.com/vi/");
  e.raw(vid, 11);
  LIT(e, "/hq.jpg\",\"media_url\":\"\",\"comments\":null,"
         "\"reactions\":null,\"outlinks\":[");
  // every distinct URL of the description, in first-appearance order
  // (oracle: convert.extract_urls)
  UrlScan u{desc, desc_n, 0, 0, 0, 0};
  unsigned long long url_keys = 0;  // url_key() of every URL so far
  int first_url = 0;
  while (u.next()) {
    const unsigned long long key = url_key(u);
    if ((url_keys & key) &&
        url_seen_before(desc, desc_n, first_url, u.start, u.len))
      continue;
    if (url_keys) LIT(e, ",");
    else first_url = u.start;
    url_keys |= key;
    LIT(e, "\"");
    e.esc(desc + u.start, u.len);
    LIT(e, "\"");
  }
  LIT(e, "],\"capture_time\":\"");
  e.raw(B.capture_str, B.capture_len);
  LIT(e, "\",\"handle\":\"");
  e.esc(ctitle, ctitle_n);
  LIT(e, "\"}\n");
  return e.cur;
}

__global__ void __launch_bounds__(256, 4)
yt_measure_kernel(YtView B, int* line_len) {
  const int wave = wave_id();
  for (int i = blockIdx.x * 4 + wave; i < B.n; i += gridDim.x * 4) {
    int len = emit_yt<false>(B, i, nullptr);
    if (lane_id() == 0) line_len[i] = len;
  }
}

__global__ void __launch_bounds__(256, 4)
yt_write_kernel(YtView B, const long* line_off, unsigned char* out) {
  const int wave = wave_id();
  for (int i = blockIdx.x * 4 + wave; i < B.n; i += gridDim.x * 4) {
    emit_yt<true>(B, i, out + line_off[i]);
  }
}

// the pointer array is laid out by views.h
static YtView yt_make_view(void** p, const long* s) {
  YtView V;
  int k = 0;
  YtView_FIELDS(VIEW_UNPACK)
  V.n = (int)s[0];
  V.label_len = (int)s[1];
  V.created_len = (int)s[2];
  V.capture_len = (int)s[3];
  return V;
}

}  // namespace crawl

extern "C" {

int crawl_yt_ptr_count() { return 0 YtView_FIELDS(VIEW_COUNT); }

int crawl_yt_measure(void** ptrs, const long* scalars, void* line_len,
                     int grid, void* stream) {
  crawl::YtView B = crawl::yt_make_view(ptrs, scalars);
  hipLaunchKernelGGL(crawl::yt_measure_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, B, (int*)line_len);
  return (int)hipGetLastError();
}

int crawl_yt_write(void** ptrs, const long* scalars, const void* line_off,
                   void* out, int grid, void* stream) {
  crawl::YtView B = crawl::yt_make_view(ptrs, scalars);
  hipLaunchKernelGGL(crawl::yt_write_kernel, dim3(grid), dim3(256), 0,
                     (hipStream_t)stream, B, (const long*)line_off,
                     (unsigned char*)out);
  return (int)hipGetLastError();
}

}  // extern "C"
