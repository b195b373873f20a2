// The pointer-array ABI between the Python drivers and the kernels' views:
// the ONE place a view's fields, their C types and their order are written.
//
// `<View>_FIELDS(F)` lists a view's pointer fields as `F(type, name)`, in
// the order the driver packs them into its `void**` array. The .hip
// sources expand a list three ways (struct members, `V.name = (type)p[k++];`
// unpacking, a field count) and ops/views.py parses this file as text to
// pack the array and check each tensor's dtype against the element type.
// A list may be split into numbered segments (`<View>_FIELDS_<n>`) where a
// struct keeps hand-written scalar members between its pointers.
//
// Keep the file to `#define`s of these two shapes: views.py rejects
// anything else inside a list.
#pragma once

// The expansions. VIEW_UNPACK and VIEW_LOCAL read the pointer array `p`
// at the running index `k`; VIEW_UNPACK fills the view `V`.
#define VIEW_MEMBER(type, name) type name;
#define VIEW_COUNT(type, name) +1
#define VIEW_UNPACK(type, name) V.name = (type)p[k++];
#define VIEW_LOCAL(type, name) type name = (type)p[k++];

// ---- BatchView (parse_encode.hip): per-message columns, pools and
// tables (entities is [E,5]: etype, off16, len16, url_off, url_len), the
// channel table, the emoji vocabulary, the preformatted Go time strings
// and the content-type name table
#define BatchView_FIELDS_0(F) \
  F(const long* __restrict__, chat_id) \
  F(const long* __restrict__, msg_id) \
  F(const long* __restrict__, text_off) \
  F(const int* __restrict__, date) \
  F(const int* __restrict__, content_type) \
  F(const int* __restrict__, views) \
  F(const int* __restrict__, forwards) \
  F(const int* __restrict__, media_album_id) \
  F(const int* __restrict__, channel_idx) \
  F(const int* __restrict__, flags) \
  F(const int* __restrict__, text_len) \
  F(const int* __restrict__, aux_off) \
  F(const int* __restrict__, aux_len) \
  F(const int* __restrict__, ent_off) \
  F(const int* __restrict__, ent_cnt) \
  F(const int* __restrict__, react_off) \
  F(const int* __restrict__, react_cnt) \
  F(const int* __restrict__, com_off) \
  F(const int* __restrict__, com_cnt) \
  F(const int* __restrict__, poster_off) \
  F(const int* __restrict__, poster_len) \
  F(const unsigned char* __restrict__, pool) \
  F(const int* __restrict__, entities) \
  F(const int* __restrict__, react_emoji) \
  F(const int* __restrict__, react_count) \
  F(const int* __restrict__, com_text_off) \
  F(const int* __restrict__, com_text_len) \
  F(const int* __restrict__, com_handle_off) \
  F(const int* __restrict__, com_handle_len) \
  F(const int* __restrict__, com_views) \
  F(const int* __restrict__, com_replies) \
  F(const int* __restrict__, com_react_off) \
  F(const int* __restrict__, com_react_cnt) \
  F(const long* __restrict__, ch_chat_id) \
  F(const int* __restrict__, ch_member) \
  F(const int* __restrict__, ch_postcount) \
  F(const int* __restrict__, ch_totalviews) \
  F(const int* __restrict__, ch_user_off) \
  F(const int* __restrict__, ch_user_len) \
  F(const int* __restrict__, ch_title_off) \
  F(const int* __restrict__, ch_title_len) \
  F(const unsigned char* __restrict__, emoji_pool) \
  F(const int* __restrict__, emoji_off) \
  F(const int* __restrict__, emoji_len) \
  F(const unsigned char* __restrict__, created_str)
#define BatchView_FIELDS_1(F) \
  F(const unsigned char* __restrict__, capture_str)
#define BatchView_FIELDS_2(F) \
  F(const unsigned char* __restrict__, ctname_pool) \
  F(const int* __restrict__, ctname_off) \
  F(const int* __restrict__, ctname_len)
#define BatchView_FIELDS(F) \
  BatchView_FIELDS_0(F) BatchView_FIELDS_1(F) BatchView_FIELDS_2(F)

// ---- LinkOut (parse_encode.hip): name [N, MAX_LINKS, 32]; name_len, src
// (0=mention 1=text_url 2=url 3=plain) and hash (fnv1a64 of the name)
// [N, MAX_LINKS]; cnt [N]
#define LinkOut_FIELDS(F) \
  F(unsigned char* __restrict__, name) \
  F(unsigned char* __restrict__, name_len) \
  F(unsigned char* __restrict__, src) \
  F(int* __restrict__, cnt) \
  F(unsigned long long* __restrict__, hash)

// ---- YtView (yt_encode.hip): lang_pool is the language codes end to end
#define YtView_FIELDS_0(F) \
  F(const int*, vid_off) \
  F(const int*, channel_idx) \
  F(const long*, published) \
  F(const long*, views) \
  F(const int*, likes) \
  F(const int*, comments) \
  F(const int*, duration_s) \
  F(const int*, lang) \
  F(const long*, title_off) \
  F(const int*, title_len) \
  F(const long*, desc_off) \
  F(const int*, desc_len) \
  F(const unsigned char*, pool) \
  F(const int*, ch_id_off) \
  F(const int*, ch_title_off) \
  F(const int*, ch_title_len) \
  F(const int*, ch_desc_off) \
  F(const int*, ch_desc_len) \
  F(const long*, ch_subs) \
  F(const int*, ch_videos) \
  F(const long*, ch_views) \
  F(const int*, ch_country_off) \
  F(const int*, ch_country_len) \
  F(const long*, ch_published) \
  F(const unsigned char*, label)
#define YtView_FIELDS_1(F) \
  F(const unsigned char*, lang_pool) \
  F(const unsigned char*, created_str)
#define YtView_FIELDS_2(F) \
  F(const unsigned char*, capture_str)
#define YtView_FIELDS(F) \
  YtView_FIELDS_0(F) YtView_FIELDS_1(F) YtView_FIELDS_2(F)

// ---- TemplateTables (feedgen.hip): concatenated template pool, aux,
// entity rows ([E_t,5]; ent_off is a ROW offset) and slot byte positions
// with their per-template [T] offsets and counts; then the comment texts
#define TemplateTables_FIELDS_0(F) \
  F(const unsigned char*, pool) \
  F(const int*, pool_off) \
  F(const int*, pool_len) \
  F(const int*, text_len) \
  F(const int*, ctype) \
  F(const int*, tflags) \
  F(const unsigned char*, aux) \
  F(const int*, aux_off) \
  F(const int*, aux_len) \
  F(const int*, ents) \
  F(const int*, ent_off) \
  F(const int*, ent_cnt) \
  F(const int*, slots) \
  F(const int*, slot_off) \
  F(const int*, slot_cnt) \
  F(const double*, cdf)
#define TemplateTables_FIELDS_1(F) \
  F(const unsigned char*, ctext) \
  F(const int*, ctext_off) \
  F(const int*, ctext_len)
#define TemplateTables_FIELDS(F) \
  TemplateTables_FIELDS_0(F) TemplateTables_FIELDS_1(F)

// ---- feedgen outputs (feedgen.hip): what each phase's kernel writes,
// in its parameter order
#define FeedMetaOut_FIELDS(F) \
  F(long*, chat_id) \
  F(long*, msg_id) \
  F(int*, date) \
  F(int*, content_type) \
  F(int*, views) \
  F(int*, forwards) \
  F(int*, media_album_id) \
  F(int*, channel_idx) \
  F(int*, flags) \
  F(int*, text_len) \
  F(int*, aux_len) \
  F(int*, ent_cnt) \
  F(int*, react_cnt) \
  F(int*, com_cnt) \
  F(int*, poster_len) \
  F(int*, reply_count) \
  F(long*, block_len) \
  F(int*, tidx)

#define FeedFillOut_FIELDS(F) \
  F(unsigned char*, pool) \
  F(long*, text_off) \
  F(int*, aux_off) \
  F(int*, poster_off) \
  F(int*, ent_off) \
  F(int*, react_off) \
  F(int*, entities) \
  F(int*, react_emoji) \
  F(int*, react_count)

#define FeedCommentOut_FIELDS(F) \
  F(unsigned char*, pool) \
  F(int*, com_text_off) \
  F(int*, com_text_len) \
  F(int*, com_handle_off) \
  F(int*, com_handle_len) \
  F(int*, com_views) \
  F(int*, com_replies) \
  F(int*, com_react_off) \
  F(int*, com_react_cnt)
